"""CPU-side checks of the regression drop-ins (audioTrainTest.regression_wrapper / file_regression / evaluate_regression,
kernels_svr.hpp, the regressor kind of kernels_forest.hpp): the NumPy restatement (tests/svr_ref.py) against the svr_* /
regforest_* goldens and the installed scikit-learn, the C ABI's names and its argument errors (reported before any device
work), and the error returns of the Python entry points.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import svr_ref
from conftest import ROOT, golden_files, golden_id
from pyaudioanalysis_amd import _ffi, audioTrainTest

SVR_SYMBOLS = ("paa_svr_create", "paa_svr_destroy", "paa_svr_num_models", "paa_svr_predict_f64", "paa_svr_dev_predict_f64")


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _golden(name):
    return _load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def _svr(g, prefix):
    return (g[prefix + "_sv"], g[prefix + "_coef"], float(g[prefix + "_intercept"]), float(g[prefix + "_gamma"]), str(g[prefix + "_kernel"]))


def _trees(g, prefix):
    return {k: g["%s_%s" % (prefix, k)] for k in ("node_offsets", "children_left", "children_right", "feature", "threshold",
                                                    "missing_go_to_left", "value")}


def test_goldens_have_their_kinds_and_no_pickles():
    names = {golden_id(f) for f in golden_files("svr")} | {golden_id(f) for f in golden_files("regforest")}
    assert names == {"svr_emotion_files", "svr_linear_files", "svr_synth", "svr_evaluate", "regforest_emotion_files"}
    for f in golden_files("svr") + golden_files("regforest"):
        g = _load(f)                                   # allow_pickle=False: arrays only
        assert str(g["sklearn_version"])


def test_restatement_matches_the_synthetic_fits():
    g = _golden("svr_synth")
    n_sv = []
    for i in range(int(g["n_models"])):
        m = _svr(g, "m%d" % i)
        got, scale = svr_ref.svr_decision(*m, g["X"], with_scale=True)
        assert np.all(np.abs(got - g["m%d_predict" % i]) <= 1e-12 * np.maximum(1.0, scale)), i
        n_sv.append(m[0].shape[0])
    assert n_sv[-1] == 0 and np.array_equal(svr_ref.svr_decision(*_svr(g, "m6"), g["X"]), np.full(g["X"].shape[0], float(g["m6_intercept"])))
    assert {str(g["m%d_kernel" % i]) for i in range(7)} == {"rbf", "linear"}


@pytest.mark.parametrize("name", ["svr_emotion_files", "svr_linear_files"])
def test_restatement_matches_the_reference_file_regression(name):
    g = _golden(name)
    assert sorted(str(t) for t in g["tasks"]) == ["arousal", "valence"] and g["lengths"].shape[0] == 4
    for t in (str(t) for t in g["tasks"]):
        X = svr_ref.standardise(g["vectors"], g[t + "_mean"], g[t + "_std"])
        got, scale = svr_ref.svr_decision(*_svr(g, t), X, with_scale=True)
        assert np.all(np.abs(got - g["sk_" + t]) <= 1e-12 * np.maximum(1.0, scale))
        assert np.all(np.abs(got - g["ref_" + t]) <= 1e-12 * np.maximum(1.0, scale))


def test_forest_restatement_matches_the_reference_file_regression():
    g = _golden("regforest_emotion_files")
    for t in (str(t) for t in g["tasks"]):
        X = svr_ref.standardise(g["vectors"], g[t + "_mean"], g[t + "_std"])
        got = svr_ref.forest_regress(_trees(g, t), X)
        assert np.array_equal(got, g["sk_" + t]) and np.array_equal(got, g["ref_" + t])


def test_restatement_matches_the_installed_scikit_learn():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.svm import SVR
    rng = np.random.default_rng(5)
    Xtr, X = rng.standard_normal((90, 17)), rng.standard_normal((40, 17))
    y = Xtr[:, 0] - 2 * Xtr[:, 3] + 0.1 * rng.standard_normal(90)
    for kernel in ("rbf", "linear"):
        m = SVR(kernel=kernel, C=2.0).fit(Xtr, y)
        got, scale = svr_ref.svr_decision(*svr_ref.svr_arrays(m), X, with_scale=True)
        assert np.all(np.abs(got - m.predict(X)) <= 1e-12 * np.maximum(1.0, scale))
    rf = RandomForestRegressor(n_estimators=7, random_state=3).fit(Xtr, y)
    X[0, 2] = np.nan
    assert np.array_equal(svr_ref.forest_regress(svr_ref.tree_arrays(rf), X), rf.predict(X))
    a = audioTrainTest.forest_arrays(rf)
    assert a.kind == "regressor" and a.n_classes == 1 and a.n_outputs == 1 and a.value.shape == a.threshold.shape
    assert not audioTrainTest.is_forest(rf) and not audioTrainTest.is_forest(a)
    two = RandomForestRegressor(n_estimators=2, random_state=0).fit(Xtr, np.stack([y, -y], axis=1))
    with pytest.raises(NotImplementedError):
        audioTrainTest.forest_arrays(two)


@pytest.mark.parametrize("method", ["svm", "randomforest"])
def test_evaluate_regression_restatement_matches_the_reference(method):
    sklearn = pytest.importorskip("sklearn")
    g = _golden("svr_evaluate")
    if sklearn.__version__ != str(g["sklearn_version"]):
        pytest.skip("golden made with scikit-learn %s, installed %s: fits need not agree" % (g["sklearn_version"], sklearn.__version__))
    np.random.seed(int(g["seed"]))
    result, printed = svr_ref.evaluate_regression(g["features"], g["labels"], int(g["n_exp"]), method, g[method + "_params"],
                                                  svr_ref.sklearn_fit, lambda m, rows: m.predict(rows))
    want = g[method + "_result"]
    assert result[0] == want[0]
    assert abs(result[1] - want[1]) <= 1e-12 * max(1.0, abs(want[1])) and abs(result[2] - want[2]) <= 1e-12 * max(1.0, abs(want[2]))
    assert printed == str(g[method + "_printed"])


def test_new_symbols_are_in_the_header_the_binding_and_the_library():
    text = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _ffi.lib()
    for s in SVR_SYMBOLS + ("paa_debug_svr_geometry",):
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert re.search(r"#define\s+PAA_FOREST_REGRESSOR\s+2\b", open(os.path.join(ROOT, "include", "paa_hip.h")).read())
    geo = np.zeros(4, dtype=np.int32)
    assert lib.paa_debug_svr_geometry(geo.ctypes.data_as(_ffi.c_i32p)) == _ffi.PAA_OK
    assert np.all(geo > 0) and lib.paa_debug_svr_geometry(None) == _ffi.ERR_ARG


def _svr_create(n_models=2, n_dims=3, offsets=(0, 2, 3), kernel=(2, 0), gamma=(0.5, 0.0), **null):
    off = np.array(offsets, dtype=np.int64)
    total = max(int(off[-1]), 1)
    sv, coef = np.ones((total, max(n_dims, 1))), np.ones(total)
    rho, gam = np.zeros(len(kernel)), np.array(gamma, dtype=np.float64)
    kt = np.array(kernel, dtype=np.int32)
    mean, std = np.zeros((len(kernel), max(n_dims, 1))), np.ones((len(kernel), max(n_dims, 1)))
    h = C.c_void_p()
    args = {"sv_offsets": _ffi.as_i64p(off), "support_vectors": _ffi.as_f64p(sv), "dual_coef": _ffi.as_f64p(coef), "rho": _ffi.as_f64p(rho),
            "kernel_type": kt.ctypes.data_as(_ffi.c_i32p), "gamma": _ffi.as_f64p(gam), "mean": _ffi.as_f64p(mean), "std": _ffi.as_f64p(std),
            "out": C.byref(h)}
    args.update(null)
    rc = _ffi.lib().paa_svr_create(n_models, args["sv_offsets"], args["support_vectors"], args["dual_coef"], args["rho"],
                                   args["kernel_type"], args["gamma"], args["mean"], args["std"], n_dims, args["out"])
    return rc, h


def test_svr_c_abi_rejects_bad_arguments_before_any_device_work():
    for name in ("sv_offsets", "support_vectors", "dual_coef", "rho", "kernel_type", "gamma", "mean", "std", "out"):
        assert _svr_create(**{name: None})[0] == _ffi.ERR_ARG, name
    assert _svr_create(n_dims=0)[0] == _ffi.ERR_ARG
    assert _svr_create(n_dims=257)[0] == _ffi.ERR_ARG
    assert _svr_create(n_models=0)[0] == _ffi.ERR_ARG
    assert _svr_create(n_models=4097)[0] == _ffi.ERR_ARG
    assert _svr_create(offsets=(0, 2, 1))[0] == _ffi.ERR_ARG                       # decreasing
    assert _svr_create(offsets=(1, 2, 3))[0] == _ffi.ERR_ARG                       # not from 0
    assert _svr_create(gamma=(0.0, 0.0))[0] == _ffi.ERR_ARG                        # RBF needs gamma > 0
    assert _svr_create(gamma=(-1.0, 0.0))[0] == _ffi.ERR_ARG
    assert _svr_create(gamma=(np.nan, 0.0))[0] == _ffi.ERR_ARG
    assert _svr_create(kernel=(1, 0))[0] == _ffi.ERR_ARG                           # polynomial
    lib = _ffi.lib()
    x, out = np.zeros(6), np.zeros(4)
    assert lib.paa_svr_predict_f64(None, _ffi.as_f64p(x), 3, 2, 2, _ffi.as_f64p(out)) == _ffi.ERR_ARG
    assert lib.paa_svr_dev_predict_f64(None, None, 3, 2, 2, None, 2) == _ffi.ERR_ARG
    assert lib.paa_svr_num_models(None) == _ffi.ERR_ARG
    assert lib.paa_svr_destroy(None) == _ffi.PAA_OK
    if _ffi.device_count() < 1:
        # a well-formed bank passes every argument test and then needs the device
        assert _svr_create()[0] not in (_ffi.PAA_OK, _ffi.ERR_ARG)
        return
    rc, h = _svr_create()                            # with a device: the matrix tests of the predict calls on a real handle
    assert rc == _ffi.PAA_OK and lib.paa_svr_num_models(h) == 2
    assert lib.paa_svr_predict_f64(h, _ffi.as_f64p(x), 3, 1, 2, _ffi.as_f64p(out)) == _ffi.ERR_ARG         # ld < n_vec
    assert lib.paa_svr_predict_f64(h, _ffi.as_f64p(x), 2, 2, 2, _ffi.as_f64p(out)) == _ffi.ERR_ARG         # wrong n_dims
    assert lib.paa_svr_predict_f64(h, _ffi.as_f64p(x), 3, 2, 0, _ffi.as_f64p(out)) == _ffi.ERR_ARG
    assert lib.paa_svr_predict_f64(h, None, 3, 2, 2, _ffi.as_f64p(out)) == _ffi.ERR_ARG
    assert lib.paa_svr_predict_f64(h, _ffi.as_f64p(x), 3, 2, 2, None) == _ffi.ERR_ARG
    assert lib.paa_svr_destroy(h) == _ffi.PAA_OK


def _forest_create(kind, n_classes, value_width):
    """One tree: a root and two leaves."""
    i64 = lambda *v: np.array(v, dtype=np.int64)                                     # noqa: E731
    off, left, right, feat = i64(0, 3), i64(1, -1, -1), i64(2, -1, -1), i64(0, -2, -2)
    thr, value, init = np.zeros(3), np.ones((3, value_width)), np.zeros(max(n_classes, 1))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    h = C.c_void_p()
    return _ffi.lib().paa_forest_create(kind, 1, ptr(off), ptr(left), ptr(right), ptr(feat), _ffi.as_f64p(thr), None,
                                        _ffi.as_f64p(value), n_classes, 2, 0.1, _ffi.as_f64p(init), C.byref(h))


def test_forest_regressor_kind_takes_exactly_one_output():
    for n_classes in (0, 2, 3):
        assert _forest_create(2, n_classes, 1) == _ffi.ERR_ARG                    # kind 2: n_classes must be 1
    for kind in (0, 1):
        assert _forest_create(kind, 1, 1) == _ffi.ERR_ARG                         # ... and only kind 2 may have 1
    assert _forest_create(3, 1, 1) == _ffi.ERR_ARG
    rc = _forest_create(2, 1, 1)                                                   # well-formed: passes the argument tests
    assert rc == _ffi.PAA_OK if _ffi.device_count() > 0 else rc not in (_ffi.PAA_OK, _ffi.ERR_ARG)


def test_regression_wrapper_of_an_unknown_type_is_none():
    assert audioTrainTest.regression_wrapper(object(), "knn", np.zeros(3)) is None
    assert audioTrainTest.regression_wrapper(object(), "gradientboosting", np.zeros(3)) is None


def test_file_regression_on_a_missing_file(capsys):
    assert audioTrainTest.file_regression("/nonexistent/clip.wav", "/nonexistent/model", "svm_rbf") == (-1, -1, -1)
    assert "wav file not found" in capsys.readouterr().out
    assert audioTrainTest.file_regression_batch(["/nonexistent/clip.wav"], "/nonexistent/model", "svm") == [(-1, -1, -1)]


def test_svr_arrays_refuse_other_kernels():
    with pytest.raises(NotImplementedError, match="SVR kernel 'poly': the GPU path serves 'rbf' and 'linear' models"):
        audioTrainTest.SvrArrays(np.zeros((1, 2)), np.zeros((1, 1)), [0.0], 0.1, "poly")
    a = audioTrainTest.SvrArrays(np.zeros((0, 2)), np.zeros((1, 0)), [0.5], 0.1, "rbf")
    assert a.support_vectors_.shape == (0, 2) and a._dual_coef_.shape == (1, 0)
    with pytest.raises(ValueError):
        audioTrainTest.ForestArrays("other", [0, 1], [-1], [-1], [0], [0.0], None, [0.0], None, 2)


def test_build_compiles_at_most_sixteen_units_at_a_time():
    from pyaudioanalysis_amd import _build
    assert "family_svr.hip" in _build.SOURCES and len(_build.SOURCES) == 18 and _build.MAX_JOBS == 16
