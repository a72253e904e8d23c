"""CPU checks of the SVM classification path (audioTrainTest / audioSegmentation.mid_term_file_classification):
the NumPy restatement of libsvm (tests/svc_libsvm.py) against scikit-learn, the host-side helpers against the reference,
the goldens' format, and no CPU fallback for the compute entry points."""
import os
import pickle

import numpy as np
import pytest

import svc_libsvm
from conftest import golden_files
from pyaudioanalysis_amd import _ffi, audioSegmentation, audioTrainTest


def _reference_segmentation():
    import load_reference
    if not load_reference.reference_available():
        pytest.skip("reference tree not present")
    return load_reference.load_segmentation()


def saturated_pairs(m, dec):
    """Number of (window, pair) Platt probabilities outside [1e-7, 1 - 1e-7], i.e. clamped by libsvm."""
    r = svc_libsvm.sigmoid_predict(dec, m["prob_a"], m["prob_b"])
    return int(np.sum((r < 1e-7) | (r > 1 - 1e-7)))


@pytest.mark.parametrize("kernel", ["rbf", "linear"])
@pytest.mark.parametrize("k", list(range(2, 17)))
def test_restatement_matches_sklearn(k, kernel):
    sklearn_svm = pytest.importorskip("sklearn.svm")
    rng = np.random.default_rng(100 * k + len(kernel))
    n_dims = int(rng.integers(3, 20))
    centres = rng.standard_normal((k, n_dims)) * 1.5
    y = np.repeat(np.arange(k), 25)
    X = centres[y] + rng.standard_normal((y.shape[0], n_dims))
    clf = sklearn_svm.SVC(kernel=kernel, probability=True, gamma="scale", random_state=0).fit(X, y)
    T = centres[rng.integers(0, k, 60)] * 0.5 + rng.standard_normal((60, n_dims))
    m = svc_libsvm.model_arrays(clf)
    idx, proba, dec = svc_libsvm.predict(m, T)
    assert np.array_equal(clf.classes_[idx], clf.predict(T))
    assert np.max(np.abs(proba - clf.predict_proba(T))) <= 1e-12
    if k == 2:              # scikit-learn's public decision_function is -(libsvm's) for two classes
        assert np.allclose(clf.decision_function(T), -dec[:, 0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("kernel", ["rbf", "linear"])
@pytest.mark.parametrize("k", list(range(2, 17)))
def test_restatement_matches_sklearn_on_separated_classes(k, kernel):
    """Clusters far apart; windows at the centres and far outside every cluster.  Linear kernel: the far windows' decision
    values are large and their Platt probabilities are clamped to [1e-7, 1 - 1e-7].  RBF: a trained model's Platt fit keeps
    |A dec + B| small (the clamp is reached only by the seeded models of tests/test_svc_gpu.py), but at the far windows
    every kernel value underflows to 0, so the decision values are exactly -rho."""
    sklearn_svm = pytest.importorskip("sklearn.svm")
    rng = np.random.default_rng(7000 + 100 * k + len(kernel))
    n_dims = int(rng.integers(3, 20))
    centres = rng.standard_normal((k, n_dims)) * 40.0
    y = np.repeat(np.arange(k), 20)
    X = centres[y] + 0.5 * rng.standard_normal((y.shape[0], n_dims))
    clf = sklearn_svm.SVC(kernel=kernel, probability=True, gamma="scale", random_state=0).fit(X, y)
    T = np.concatenate([centres[rng.integers(0, k, 40)] + 0.5 * rng.standard_normal((40, n_dims)),
                        1e3 * rng.standard_normal((8, n_dims))])
    m = svc_libsvm.model_arrays(clf)
    idx, proba, dec = svc_libsvm.predict(m, T)
    if kernel == "linear":
        assert saturated_pairs(m, dec[40:]) > 0
    else:
        assert np.array_equal(dec[40:], np.broadcast_to(-m["rho"], dec[40:].shape))
    assert np.array_equal(clf.classes_[idx], clf.predict(T))
    assert np.max(np.abs(proba - clf.predict_proba(T))) <= 1e-12


def test_svc_goldens_are_plain_arrays():
    files = golden_files("svc")
    assert len(files) >= 4
    for f in files:
        assert os.path.getsize(f) < 1000000, f          # small test vectors only
        with np.load(f, allow_pickle=False) as z:
            assert str(z["kind"]) == "svc"
            assert z["class_names"].dtype.kind == "U"
            k = z["n_support"].shape[0]
            assert z["dual_coef"].shape == (k - 1, z["sv"].shape[0])
            assert z["rho"].shape == z["prob_a"].shape == (k * (k - 1) // 2,)


def test_module_surface():
    for name in ("load_model", "classifier_wrapper", "file_classification", "file_classification_batch"):
        assert callable(getattr(audioTrainTest, name))
    for name in ("mid_term_file_classification", "labels_to_segments", "segments_to_labels", "read_segmentation_gt",
                 "load_ground_truth", "calculate_confusion_matrix"):
        assert callable(getattr(audioSegmentation, name))


def _write_model(tmp_path):
    sklearn_svm = pytest.importorskip("sklearn.svm")
    rng = np.random.default_rng(7)
    X = rng.standard_normal((60, 5))
    y = np.repeat(np.arange(3), 20).astype(float)
    clf = sklearn_svm.SVC(kernel="rbf", probability=True, random_state=0).fit(X + y[:, None], y)
    path = str(tmp_path / "svm_model")
    with open(path, "wb") as f:
        pickle.dump(clf, f)
    with open(path + "MEANS", "wb") as f:
        for obj in (list(X.mean(0)), list(X.std(0)), ["x", "y", "z"], 1.0, 0.5, 0.05, 0.025, False):
            pickle.dump(obj, f)
    return path, clf


def test_load_model_matches_reference(tmp_path):
    path, clf = _write_model(tmp_path)
    ours = audioTrainTest.load_model(path)
    assert isinstance(ours[1], np.ndarray) and ours[3] == ["x", "y", "z"] and ours[4:] == (1.0, 0.5, 0.05, 0.025, False)
    assert np.array_equal(ours[0].support_vectors_, clf.support_vectors_)
    ref_seg = _reference_segmentation()
    from pyAudioAnalysis import audioTrainTest as ref_at
    theirs = ref_at.load_model(path)
    assert np.array_equal(ours[1], theirs[1]) and np.array_equal(ours[2], theirs[2]) and ours[3:] == theirs[3:]
    assert ref_seg is not None


@pytest.mark.parametrize("labels", [[0.0], [1.0, 1.0, 0.0, 0.0, 2.0], [3.0, 3.0, 3.0], list(np.random.default_rng(3).integers(0, 4, 50) * 1.0)])
def test_label_and_segment_conversions_match_reference(labels, tmp_path):
    ours = audioSegmentation.labels_to_segments(np.array(labels), 0.5)
    gt = tmp_path / "gt.segments"
    gt.write_text("0\t1.2\tspeech\n1.2\t3.5\tmusic\n3.5\t4.0\tspeech\n")
    s, e, lab = audioSegmentation.read_segmentation_gt(str(gt))
    assert list(s) == [0, 1.2, 3.5] and lab == ["speech", "music", "speech"]
    flags, names = audioSegmentation.segments_to_labels(s, e, lab, 0.5)
    assert [names[f] for f in flags] == ["speech", "speech", "music", "music", "music", "music", "music", "speech"]
    cm = audioSegmentation.calculate_confusion_matrix(np.array([0, 1, 1]), np.array([0, 1, 0]), ["a", "b"])
    assert cm.tolist() == [[1, 1], [0, 1]]
    ref = _reference_segmentation()
    theirs = ref.labels_to_segments(np.array(labels), 0.5)
    assert np.array_equal(np.asarray(ours[0]), np.asarray(theirs[0])) and list(ours[1]) == list(theirs[1])
    rs, re_, rl = ref.read_segmentation_gt(str(gt))
    assert np.array_equal(rs, s) and np.array_equal(re_, e) and rl == lab
    rflags, rnames = ref.segments_to_labels(rs, re_, rl, 0.5)
    assert [rnames[f] for f in rflags] == [names[f] for f in flags]
    assert np.array_equal(ref.calculate_confusion_matrix(np.array([0, 1, 1]), np.array([0, 1, 0]), ["a", "b"]), cm)


def test_compute_entry_points_have_no_cpu_fallback(tmp_path):
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present")
    path = golden_files("svc")[0]
    with np.load(path, allow_pickle=False) as z:
        model = audioTrainTest.SvcArrays(z["sv"], z["n_support"], z["dual_coef"], -z["rho"], z["prob_a"], z["prob_b"],
                                         z["gamma"], str(z["kernel"]), z["classes"])
        n_dims = z["sv"].shape[1]
    with pytest.raises(_ffi.HipLibraryError):
        audioTrainTest.svm_predict(model, np.zeros((n_dims, 3)), np.zeros(n_dims), np.ones(n_dims))
    with pytest.raises(_ffi.HipLibraryError):
        audioTrainTest.classifier_wrapper(model, "svm_rbf", np.zeros(n_dims))
    with pytest.raises(_ffi.HipLibraryError):
        audioSegmentation.mid_term_labels(np.zeros(32000, dtype=np.int16), 16000, model, np.zeros(n_dims), np.ones(n_dims),
                                          1.0, 1.0, 0.05, 0.05)


def test_c_abi_rejects_unsupported_models():
    """-1 (PAA_ERR_ARG) for k outside 2..16, dims outside 1..256 or a kernel other than LINEAR / RBF -- checked before
    any device work, so this holds with and without a GPU."""
    import ctypes as C
    lib = _ffi.lib()
    sv = np.zeros((4, 3))
    coef = np.zeros((16, 4))
    pr = np.zeros(200)
    h = C.c_void_p()

    def create(n_support, k, n_dims, kernel):
        ns = np.asarray(n_support, dtype=np.int32)
        return lib.paa_svc_create(_ffi.as_f64p(sv), 4, n_dims, ns.ctypes.data_as(_ffi.c_i32p), k, _ffi.as_f64p(coef),
                                  _ffi.as_f64p(pr), _ffi.as_f64p(pr), _ffi.as_f64p(pr), kernel, 0.5, C.byref(h))
    assert create([4], 1, 3, 2) == _ffi.ERR_ARG
    assert create([1] * 17, 17, 3, 2) == _ffi.ERR_ARG
    assert create([2, 2], 2, 257, 2) == _ffi.ERR_ARG
    assert create([2, 2], 2, 3, 1) == _ffi.ERR_ARG           # POLY
    assert create([2, 1], 2, 3, 2) == _ffi.ERR_ARG           # n_support does not sum to n_sv
    assert lib.paa_svc_predict_f64(None, _ffi.as_f64p(sv), 3, 1, 1, _ffi.as_f64p(pr), _ffi.as_f64p(pr), None, None) == _ffi.ERR_ARG


@pytest.mark.parametrize("model", ["svm_rbf_speaker_10", "svm_rbf_movie8class"])
def test_restatement_matches_sklearn_on_the_large_shipped_models(model):
    """The two shipped models whose arrays are too large for a golden file: on the reference's own mid-term features of
    diarizationExample.wav, the restatement (which the GPU tests hold the kernel against on models of exactly these shapes)
    equals scikit-learn's predict and predict_proba."""
    import warnings
    _reference_segmentation()
    from pyAudioAnalysis import MidTermFeatures as ref_mtf, audioBasicIO as ref_io, audioTrainTest as ref_at
    import load_reference
    path = os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", "models", model)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf, mean, std, _, mt_win, mid_step, st_win, st_step, _ = ref_at.load_model(path)
    fs, sig = ref_io.read_audio_file(os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data",
                                                  "diarizationExample.wav"))
    sig = ref_io.stereo_to_mono(sig)[:20 * fs]
    mt, _, _ = ref_mtf.mid_feature_extraction(sig, fs, mt_win * fs, mid_step * fs, round(fs * st_win), round(fs * st_step))
    X = (mt.T - mean) / std
    m = svc_libsvm.model_arrays(clf)
    assert tuple(m["n_support"]) == {"svm_rbf_speaker_10": svc_libsvm.SPEAKER_10_N_SUPPORT,
                                     "svm_rbf_movie8class": svc_libsvm.MOVIE8CLASS_N_SUPPORT}[model]
    idx, proba, _ = svc_libsvm.predict(m, X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(clf.classes_[idx], clf.predict(X))
        assert np.max(np.abs(proba - clf.predict_proba(X))) <= 1e-12
