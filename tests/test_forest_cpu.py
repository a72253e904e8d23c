"""CPU checks of the tree-ensemble classification path ("randomforest", "extratrees", "gradientboosting"): the NumPy
restatement (tests/forest_ref.py) against the installed scikit-learn and the goldens' recorded reference outputs, the
goldens' format, the C ABI's model validation, and the model types' reach into every file-level entry point."""
import ctypes as C
import os
import pickle
import warnings

import numpy as np
import pytest

import forest_ref
from conftest import golden_files, golden_id
from pyaudioanalysis_amd import _ffi, audioSegmentation, audioTrainTest


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_model(g):
    return audioTrainTest.ForestArrays(str(g["ens_kind"]), g["node_offsets"], g["children_left"], g["children_right"],
                                       g["feature"], g["threshold"], g["missing_go_to_left"], g["value"], g["classes"],
                                       int(g["n_dims"]), float(g["learning_rate"]),
                                       g["init"] if str(g["ens_kind"]) == "boosted" else None)


def _fit(kind, n_classes, seed):
    ens = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((500, 7))
    y = np.floor(np.clip(X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(500), -1.99, 1.99) * n_classes / 4 +
                 n_classes / 2).astype(np.float64)
    cls = {"randomforest": lambda: ens.RandomForestClassifier(n_estimators=12, random_state=seed),
           "extratrees": lambda: ens.ExtraTreesClassifier(n_estimators=12, random_state=seed),
           "gradientboosting": lambda: ens.GradientBoostingClassifier(n_estimators=15, random_state=seed)}[kind]()
    cls.fit(X, y)
    assert cls.classes_.shape[0] == n_classes
    return cls


def _queries(model, rng, nan):
    Q = rng.standard_normal((3000, model.n_features_in_)) * 1.3
    if nan:
        Q[::7, rng.integers(0, Q.shape[1])] = np.nan
    a = audioTrainTest.forest_arrays(model)
    Q[1::11] = forest_ref.tie_rows(a, Q[1::11].shape[0], rng, Q[1::11])       # float32 values equal to thresholds
    return Q


@pytest.mark.parametrize("n_classes", [2, 3, 8])
@pytest.mark.parametrize("kind", ["randomforest", "extratrees", "gradientboosting"])
def test_restatement_is_bit_identical_to_scikit_learn(kind, n_classes):
    model = _fit(kind, n_classes, 11 + n_classes)
    a = audioTrainTest.forest_arrays(model)
    rng = np.random.default_rng(n_classes)
    boosted = kind == "gradientboosting"
    Q = _queries(model, rng, nan=not boosted)
    labels, proba, raw = forest_ref.predict(a, Q)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(a.classes_[labels], model.predict(Q))
        if boosted:
            assert np.array_equal(raw.reshape(-1) if n_classes == 2 else raw, model.decision_function(Q))
            assert np.max(np.abs(proba - model.predict_proba(Q))) <= 1e-15
        else:
            assert np.array_equal(proba, model.predict_proba(Q))
        # rule 2: the same ValueError for the whole call
        for bad, message in ((1e300, forest_ref.INF_MESSAGE), (-np.inf, forest_ref.INF_MESSAGE),
                             (np.nan, forest_ref.NAN_MESSAGE if boosted else None)):
            B = Q[:50].copy()
            B[3, 2] = bad
            if message is None:
                model.predict_proba(B)
                forest_ref.predict(a, B)
                continue
            with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
                model.predict_proba(B)
            with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
                forest_ref.predict(a, B)
        # +-3.4028235e38 rounds to float32's largest value and passes
        B = Q[:20].copy()
        B[:, 0] = 3.4028235e38
        B[:10, 1] = -3.4028235e38
        labels, proba, _ = forest_ref.predict(a, B)
        assert np.array_equal(a.classes_[labels], model.predict(B))


def test_forest_goldens_are_plain_arrays():
    files = golden_files("forest")
    assert len(files) >= 7
    kinds, cases = set(), set()
    for f in files:
        assert os.path.getsize(f) < 1000000, f
        with np.load(f, allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files)
            assert z["class_names"].dtype.kind == "U"
            assert z["mid"].shape[0] == int(z["n_dims"]) == z["edge_X"].shape[1]
            kinds.add(str(z["model_type"]))
            cases.add(str(z["case"]))
            assert z["edge_X"].shape[0] == 24
    assert kinds == {"randomforest", "extratrees", "gradientboosting"} and cases == {"segment", "file"}


@pytest.mark.parametrize("path", golden_files("forest"), ids=golden_id)
def test_restatement_reproduces_golden(path):
    g = _load(path)
    a = golden_model(g)
    boosted = a.kind == "boosted"
    for X, lab, prob, raw in (((g["mid"].T - g["mean"]) / g["std"], g["ref_labels"], g["ref_proba"], g["ref_raw"]),
                              (g["edge_X"], g["edge_labels"], g["edge_proba"], g["edge_raw"])):
        labels, proba, r = forest_ref.predict(a, X)
        assert np.array_equal(a.classes_[labels], lab)
        if boosted:
            assert np.array_equal(r, raw) and np.max(np.abs(proba - prob)) <= 1e-15
        else:
            assert np.array_equal(proba, prob)
    assert str(g["nan_error"]).startswith(forest_ref.NAN_MESSAGE) if boosted else str(g["nan_error"]) == ""
    assert str(g["inf_error"]).startswith(forest_ref.INF_MESSAGE)
    if not boosted:
        assert np.isnan(g["edge_X"]).any()
    if str(g["case"]) == "file":
        assert np.array_equal(g["ref_labels"], g["ref_ids"])


def _create(a, kind=None, n_classes=None, n_dims=None, n_trees=None):
    lib = _ffi.lib()
    h = C.c_void_p()
    ptr = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)             # noqa: E731
    init = np.zeros(max(1, a.n_outputs if a.kind == "boosted" else 1))
    arrays = [np.ascontiguousarray(x) for x in (a.node_offsets, a.children_left, a.children_right, a.feature,
                                                a.missing_go_to_left)]
    rc = lib.paa_forest_create(kind if kind is not None else (1 if a.kind == "boosted" else 0),
                               n_trees if n_trees is not None else a.node_offsets.shape[0] - 1,
                               ptr(arrays[0]), ptr(arrays[1]), ptr(arrays[2]), ptr(arrays[3]), _ffi.as_f64p(a.threshold),
                               ptr(arrays[4]), _ffi.as_f64p(a.value), n_classes if n_classes is not None else a.n_classes,
                               n_dims if n_dims is not None else a.n_dims, 0.1, _ffi.as_f64p(init), C.byref(h))
    return rc


def _small(kind="averaged", n_classes=3, n_dims=5):
    return forest_ref.synthetic_forest(kind, 3, 9, 4, n_classes, n_dims, 5)


def test_c_abi_rejects_malformed_models():
    """PAA_ERR_ARG for every malformed model -- checked on the host before any device work, so this holds with and
    without a GPU."""
    def mutated(**change):
        a = _small()
        for k, fn in change.items():
            setattr(a, k, fn(getattr(a, k).copy()))
        return a

    def set_at(i, v):
        def f(x):
            x[i] = v
            return x
        return f
    a = _small()
    internal = int(np.flatnonzero(a.children_left[:a.node_offsets[1]] != -1)[-1])
    assert _create(mutated(children_right=set_at(internal, 0))) == _ffi.ERR_ARG                   # a cycle to the root
    assert _create(mutated(children_left=set_at(internal, 10 ** 6))) == _ffi.ERR_ARG              # child out of range
    assert _create(mutated(children_left=set_at(internal, -5))) == _ffi.ERR_ARG
    assert _create(mutated(feature=set_at(internal, 5))) == _ffi.ERR_ARG                          # feature >= dims
    assert _create(mutated(feature=set_at(internal, -1))) == _ffi.ERR_ARG
    shared = mutated()
    shared.children_left[internal] = shared.children_right[internal]                              # a node reached twice
    assert _create(shared) == _ffi.ERR_ARG
    assert _create(a, n_classes=1) == _ffi.ERR_ARG
    assert _create(a, n_classes=65) == _ffi.ERR_ARG
    assert _create(a, n_dims=257) == _ffi.ERR_ARG
    assert _create(a, n_dims=0) == _ffi.ERR_ARG
    assert _create(a, n_trees=0) == _ffi.ERR_ARG                                                  # empty forest
    assert _create(a, kind=7) == _ffi.ERR_ARG
    b = _small("boosted", n_classes=3)
    assert _create(b, n_trees=b.node_offsets.shape[0] - 2) == _ffi.ERR_ARG                        # not whole stages
    empty_tree = _small()
    empty_tree.node_offsets[1] = empty_tree.node_offsets[0]
    assert _create(empty_tree) == _ffi.ERR_ARG
    lib = _ffi.lib()
    x = np.zeros(3)
    idx = np.zeros(1, dtype=np.int32)
    assert lib.paa_forest_predict_f64(None, _ffi.as_f64p(x), 3, 1, 1, _ffi.as_f64p(x), _ffi.as_f64p(x),
                                      idx.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(x), None) == _ffi.ERR_ARG
    assert lib.paa_forest_dev_predict_f64(None, None, 3, 1, 1, None, None, None, None, None) == _ffi.ERR_ARG
    assert lib.paa_forest_num_classes(None) == _ffi.ERR_ARG
    assert lib.paa_forest_destroy(None) == _ffi.PAA_OK


def test_python_side_rejects_inconsistent_arrays():
    a = _small()
    a.value = a.value[:, :2]
    with pytest.raises(ValueError):
        audioTrainTest.ForestModel(a)
    with pytest.raises(ValueError):
        audioTrainTest.ForestArrays("stacked", [0, 1], [-1], [-1], [0], [0.0], None, [[1.0, 0.0]], [0, 1], 1)


def test_module_surface():
    for name in ("ForestArrays", "ForestModel", "forest_arrays", "forest_model", "forest_predict", "is_forest"):
        assert callable(getattr(audioTrainTest, name))


def test_unsupported_boosting_init_is_refused():
    ens = pytest.importorskip("sklearn.ensemble")
    from sklearn.linear_model import LogisticRegression
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 4))
    y = (X[:, 0] > 0).astype(float)
    gb = ens.GradientBoostingClassifier(n_estimators=5, init=LogisticRegression()).fit(X, y)
    with pytest.raises(NotImplementedError):
        audioTrainTest.forest_arrays(gb)
    zero = ens.GradientBoostingClassifier(n_estimators=5, init="zero").fit(X, y)
    assert np.array_equal(audioTrainTest.forest_arrays(zero).init, [0.0])


@pytest.mark.parametrize("kind", ["randomforest", "extratrees", "gradientboosting"])
def test_forest_model_types_reach_the_loader(kind, tmp_path):
    """Every file-level entry point accepts the three model types (no NotImplementedError) and loads the model as the
    reference does; without a device the computation then raises HipLibraryError."""
    model = _fit(kind, 2, 4)
    path = str(tmp_path / "model")
    with open(path, "wb") as f:
        pickle.dump(model, f)
    with open(path + "MEANS", "wb") as f:
        for obj in (np.zeros(7), np.ones(7), ["a", "b"], 1.0, 1.0, 0.05, 0.05, False):
            pickle.dump(obj, f)
    loaded = audioTrainTest.load_model(path)
    assert type(loaded[0]) is type(model) and audioTrainTest.is_forest(loaded[0])
    wav = str(tmp_path / "x.wav")
    import scipy.io.wavfile as wavfile
    wavfile.write(wav, 16000, (1000 * np.sin(np.arange(48000) * 0.05)).astype(np.int16))
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present: the GPU suite runs these entry points")
    calls = [lambda: audioTrainTest.file_classification(wav, path, kind),
             lambda: audioTrainTest.file_classification_batch([wav], path, kind),
             lambda: audioSegmentation.mid_term_file_classification(wav, path, kind),
             lambda: audioTrainTest.classifier_wrapper(model, kind, np.zeros(7))]
    for call in calls:
        with pytest.raises(_ffi.HipLibraryError):
            call()
