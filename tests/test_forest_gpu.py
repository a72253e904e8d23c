"""GPU tests of the tree-ensemble classifiers (kernels_forest.hpp) and the "randomforest" / "extratrees" /
"gradientboosting" model types of the classification drop-ins, against the forest_* goldens (scikit-learn models trained
by the unmodified reference, scripts/make_forest_golden.py) and the NumPy restatement (tests/forest_ref.py).  Reads
neither the reference tree nor scikit-learn: models come as plain arrays (audioTrainTest.ForestArrays)."""
import contextlib
import io
import tempfile

import numpy as np
import pytest

import forest_ref
from conftest import golden_files, golden_id
from pyaudioanalysis_amd import MidTermFeatures, _ffi, audioSegmentation, audioTrainTest

pytestmark = pytest.mark.gpu


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _model(g):
    boosted = str(g["ens_kind"]) == "boosted"
    return audioTrainTest.ForestArrays(str(g["ens_kind"]), g["node_offsets"], g["children_left"], g["children_right"],
                                       g["feature"], g["threshold"], g["missing_go_to_left"], g["value"], g["classes"],
                                       int(g["n_dims"]), float(g["learning_rate"]), g["init"] if boosted else None)


def _by_case(case):
    return [f for f in golden_files("forest") if str(np.load(f, allow_pickle=False)["case"]) == case]


def _agrees(a, labels, proba, raw, want_labels, want_proba, want_raw):
    """RF / ET: labels and probabilities bit for bit; GB: labels and raw scores bit for bit, probabilities to 1e-14."""
    assert np.array_equal(a.classes_[labels], want_labels)
    if a.kind == "boosted":
        assert np.array_equal(raw, want_raw)
        assert np.max(np.abs(proba - want_proba)) <= 1e-14
    else:
        assert np.array_equal(proba, want_proba)


@pytest.mark.parametrize("path", golden_files("forest"), ids=golden_id)
def test_forest_kernel_matches_scikit_learn(gpu_lib, path):
    g = _load(path)
    a = _model(g)
    model = audioTrainTest.forest_model(a)
    labels, proba, raw = model.predict(g["mid"], g["mean"], g["std"], raw=True)
    _agrees(a, labels, proba, raw, g["ref_labels"], g["ref_proba"], g["ref_raw"])
    # NaN rows (forests: the missing-value branch), +-FLT_MAX, float32 values at the thresholds
    E = g["edge_X"]
    n = E.shape[0]
    labels, proba, raw = model.predict(E.T, np.zeros(E.shape[1]), np.ones(E.shape[1]), raw=True)
    _agrees(a, labels, proba, raw, g["edge_labels"], g["edge_proba"], g["edge_raw"])
    print("%s: %d vectors + %d edge rows" % (golden_id(path), g["mid"].shape[1], n))
    # the public one-vector form equals the batch
    X = (g["mid"].T - g["mean"]) / g["std"]
    ids, P = audioTrainTest.forest_predict(a, g["mid"], g["mean"], g["std"])
    kind = str(g["model_type"])
    for v in range(0, X.shape[0], max(1, X.shape[0] // 9)):
        cid, p = audioTrainTest.classifier_wrapper(a, kind, X[v])
        assert cid == ids[v] and np.array_equal(p, P[v])
    # rule 2: scikit-learn's ValueError for the whole call
    bad = g["mid"].copy()
    bad[0, 1] = 1e300 * g["std"][0]
    with pytest.raises(ValueError, match=r"Input X contains infinity or a value too large for dtype\('float32'\)"):
        model.predict(bad, g["mean"], g["std"])
    bad[0, 1] = np.nan
    if a.kind == "boosted":
        assert str(g["nan_error"]).startswith("Input X contains NaN")
        with pytest.raises(ValueError, match="Input X contains NaN"):
            model.predict(bad, g["mean"], g["std"])
    else:
        assert str(g["nan_error"]) == ""
        model.predict(bad, g["mean"], g["std"])


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
    kind = str(g["model_type"])
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        labels, class_names, acc, cm = audioSegmentation.mid_term_classification(
            g["signal"], g["fs"], _model(g), g["mean"], g["std"], names, float(g["mt_win"]), float(g["mid_step"]),
            float(g["st_win"]), float(g["st_step"]), False, False, gt_file, kind)
    assert class_names == names
    assert np.array_equal(labels, g["seg_labels"])
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


@pytest.mark.parametrize("path", _by_case("file"), ids=golden_id)
def test_file_classification_matches_reference(gpu_lib, path):
    g = _load(path)
    kind = str(g["model_type"])
    args = (_model(g), g["mean"], g["std"], float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]), float(g["st_step"]),
            bool(g["compute_beat"]))
    pos, sigs = 0, []
    for n, cid, prob in zip(g["lengths"], g["ref_ids"], g["ref_file_proba"]):
        sig = g["signals"][pos:pos + int(n)]
        pos += int(n)
        sigs.append(sig)
        ours, p = audioTrainTest.file_classification_signal(sig, g["fs"], *args, kind)
        assert ours == cid
        if kind == "gradientboosting":
            assert np.max(np.abs(p - prob)) <= 1e-14
        else:
            assert np.array_equal(p, prob)
    ids, proba = audioTrainTest.file_classification_signals(sigs, int(g["fs"]), *args, kind)
    assert np.array_equal(ids, g["ref_ids"])
    assert np.max(np.abs(proba - g["ref_file_proba"])) <= (1e-14 if kind == "gradientboosting" else 0.0)


@pytest.mark.parametrize("path", _by_case("file"), ids=golden_id)
def test_file_classification_batch_equals_single_calls(gpu_lib, path):
    g = _load(path)
    kind = str(g["model_type"])
    rng = np.random.default_rng(12)
    fs = int(g["fs"])
    sigs = []
    for i in range(40):
        n = int(rng.integers(int(0.3 * fs), int(5.0 * fs)))
        t = np.arange(n) / fs
        x = 6000 * np.sin(2 * np.pi * rng.uniform(80, 2000) * t) * (1 + np.sin(2 * np.pi * rng.uniform(0.5, 4) * t))
        x += rng.normal(0, rng.uniform(50, 3000), n)
        sigs.append(np.clip(x, -32768, 32767).astype(np.int16))
    args = (_model(g), g["mean"], g["std"], float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]),
            float(g["st_step"]), bool(g["compute_beat"]))
    ids, proba = audioTrainTest.file_classification_signals(sigs, fs, *args, kind)
    for i, s in enumerate(sigs):
        cid, p = audioTrainTest.file_classification_signal(s, fs, *args, kind)
        assert cid == ids[i] and np.array_equal(p, proba[i]), i


def test_file_level_entry_points_with_model_files(gpu_lib, tmp_path):
    """mid_term_file_classification, file_classification and file_classification_batch on model files: the pickled model
    is the golden's ForestArrays (what load_model unpickles is only read through its arrays)."""
    import pickle
    import scipy.io.wavfile as wavfile
    g = _load(_by_case("segment")[0])
    kind = str(g["model_type"])
    model = str(tmp_path / "model")
    with open(model, "wb") as f:
        pickle.dump(_model(g), f)
    with open(model + "MEANS", "wb") as f:
        for obj in (g["mean"], g["std"], [str(c) for c in g["class_names"]], float(g["mt_win"]), float(g["mid_step"]),
                    float(g["st_win"]), float(g["st_step"]), False):
            pickle.dump(obj, f)
    wav = str(tmp_path / "signal.wav")
    wavfile.write(wav, int(g["fs"]), g["signal"])
    with contextlib.redirect_stdout(io.StringIO()):
        labels, class_names, acc, cm = audioSegmentation.mid_term_file_classification(wav, model, kind, False, "")
    assert np.array_equal(labels, g["seg_labels"])
    one = audioTrainTest.file_classification(wav, model, kind)
    batch = audioTrainTest.file_classification_batch([wav, wav], model, kind)
    for cid, p, names in batch:
        assert cid == one[0] and np.array_equal(p, one[1]) and names == one[2]


def _check_restatement(a, feats, mean, std, what):
    X = (feats.T - mean) / std
    labels, proba, raw = audioTrainTest.forest_model(a).predict(feats, mean, std, raw=True)
    want_labels, want_proba, want_raw = forest_ref.predict(a, X, check=False)
    assert np.array_equal(labels, want_labels), what
    assert np.array_equal(raw, want_raw), what
    if a.kind == "boosted":
        assert np.max(np.abs(proba - want_proba)) <= 1e-14, what
    else:
        assert np.array_equal(proba, want_proba), what
    print("%s: %d vectors, labels used %s" % (what, X.shape[0], np.unique(labels).tolist()))


SEEDED = {
    # name: (kind, n_trees / stages, nodes per tree, max depth, classes, dims, n_vec, chain depth)
    "et25_movie8class_shape": ("averaged", 25, (2000, 3400), 33, 8, 136, 2111, 0),
    "rf500_movie8class_shape": ("averaged", 500, (800, 1500), 27, 8, 136, 3001, 0),
    "gb100x8_movie8class_shape": ("boosted", 100, (7, 15), 3, 8, 136, 2111, 0),
    "gb100_binary": ("boosted", 100, (7, 15), 3, 2, 136, 777, 0),
    "c64_d256": ("averaged", 20, (100, 400), 14, 64, 256, 1000, 0),
    "one_dim": ("averaged", 30, (1, 61), 9, 3, 1, 500, 0),
    "single_leaf_trees": ("averaged", 12, 1, 0, 4, 10, 300, 0),
    "chain_2000": ("averaged", 3, (5, 31), 6, 3, 12, 400, 2000),
    "gb_chain_2000": ("boosted", 4, (5, 31), 6, 3, 12, 400, 2000),
}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_seeded_models_match_restatement(gpu_lib, name):
    kind, n_trees, n_nodes, depth, n_classes, n_dims, n_vec, chain = SEEDED[name]
    a = forest_ref.synthetic_forest(kind, n_trees, n_nodes, depth, n_classes, n_dims, 40 + len(name), chain_depth=chain)
    rng = np.random.default_rng(41)
    mean, std = rng.normal(0, 1, n_dims), rng.uniform(0.5, 2.0, n_dims)
    X = rng.standard_normal((n_vec, n_dims)) * 1.2
    if chain:
        X[: n_vec // 4] = rng.uniform(3.5, 5.0, (n_vec // 4, n_dims))         # walk the whole chain
    X[1::13] = forest_ref.tie_rows(a, X[1::13].shape[0], rng, X[1::13])      # float32 values equal to thresholds
    if kind == "averaged":
        X[2::17, rng.integers(0, n_dims)] = np.nan
    # the FP64 standardisation must give back exactly the tie values: feed them with mean 0, std 1
    _check_restatement(a, (X * std + mean).T, mean, std, name)
    _check_restatement(a, X.T.copy(), np.zeros(n_dims), np.ones(n_dims), name + " (ties exact)")


def test_invalid_values_follow_rule_two(gpu_lib):
    """Per-vector codes through the C ABI: -1 where a value overflows float32, -2 for NaN under boosting; forests follow
    the missing-value branch; +-3.4028235e38 passes."""
    rng = np.random.default_rng(8)
    for kind in ("averaged", "boosted"):
        a = forest_ref.synthetic_forest(kind, 10, (9, 41), 6, 3, 6, 3)
        m = audioTrainTest.forest_model(a)
        X = rng.standard_normal((12, 6))
        X[1, 2] = 1e300
        X[2, 0] = -1e39
        X[3, 4] = np.nan
        X[4, :] = 3.4028235e38
        X[5, :] = -3.4028235e38
        X[6, 1] = np.inf
        F = np.ascontiguousarray(X.T)
        idx = np.empty(12, dtype=np.int32)
        P = np.empty((12, 3))
        _ffi.check(_ffi.lib().paa_forest_predict_f64(m.handle, _ffi.as_f64p(F), 6, 12, 12, _ffi.as_f64p(np.zeros(6)),
                                                     _ffi.as_f64p(np.ones(6)), idx.ctypes.data_as(_ffi.c_i32p),
                                                     _ffi.as_f64p(P), None))
        want, wP, _ = forest_ref.predict(a, X, check=False)
        assert np.array_equal(idx, want)
        assert idx[1] == idx[2] == idx[6] == -1
        assert idx[3] == (-2 if kind == "boosted" else want[3]) and idx[4] >= 0 and idx[5] >= 0
        ok = idx >= 0
        assert np.array_equal(P[ok], wP[ok]) if kind == "averaged" else np.max(np.abs(P[ok] - wP[ok])) <= 1e-14
        with pytest.raises(ValueError):
            m.predict(X.T, np.zeros(6), np.ones(6))


def test_one_hour_clip_through_the_device_path(gpu_lib):
    """A 1-hour 16 kHz clip at a 1 s mid-term step through mid_term_labels (the mid-term matrix goes from the plan straight
    into the traversal kernel) against the host-buffer path and, on a sample, the restatement; RandomForest-100 at
    knn_movie8class's shape, then GradientBoosting-100 x 8."""
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
    for kind, model_type, trees, nodes, depth in (("averaged", "randomforest", 100, (800, 1500), 27),
                                                  ("boosted", "gradientboosting", 100, (7, 15), 3)):
        a = forest_ref.synthetic_forest(kind, trees, nodes, depth, 8, mid.shape[0], 77)
        labels_dev, pmax_dev = audioSegmentation.mid_term_labels(sig, fs, a, mean, std, mt_win, mid_step, st_win, st_step,
                                                                 model_type)
        assert mid.shape[1] == labels_dev.shape[0] >= 3500
        labels_host, P_host = audioTrainTest.forest_predict(a, mid, mean, std)
        assert np.array_equal(labels_host, labels_dev) and np.array_equal(P_host.max(axis=1), pmax_dev)
        pick = np.sort(rng.choice(mid.shape[1], 300, replace=False))
        _check_restatement(a, mid[:, pick], mean, std, "1 h, %s" % model_type)
