"""GPU tests of the regression drop-ins (kernels_svr.hpp, the regressor kind of kernels_forest.hpp; audioTrainTest.regress /
regression_wrapper / file_regression_* / evaluate_regression, audioSegmentation.mid_term_regression_signal) against the
svr_* / regforest_* goldens (scikit-learn models trained by the unmodified reference, scripts/make_regress_golden.py) and
the NumPy restatement (tests/svr_ref.py).  Models come as plain arrays (SvrArrays / ForestArrays); only the
evaluate_regression test needs scikit-learn.

Bound of the SVR values: |ours - scikit-learn| <= 1e-9 max(1, scale(v)), scale(v) = sum_s |coef_s K_s(v)| + |intercept| --
the project's tight gate; the restatement sits at about 1e-15 of scikit-learn.  Forest regressors: bit for bit."""
import contextlib
import io
import os

import numpy as np
import pytest

import svr_ref
from conftest import ROOT
from pyaudioanalysis_amd import MidTermFeatures, audioSegmentation, audioTrainTest

pytestmark = pytest.mark.gpu
_cache = {}


def _golden(name):
    if name not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def _svr_tuple(g, prefix):
    return (g[prefix + "_sv"], g[prefix + "_coef"], float(g[prefix + "_intercept"]), float(g[prefix + "_gamma"]), str(g[prefix + "_kernel"]))


def _svr(g, prefix):
    sv, coef, intercept, gamma, kernel = _svr_tuple(g, prefix)
    return audioTrainTest.SvrArrays(sv, coef, [intercept], gamma, kernel)


def _forest(g, prefix):
    a = {k: g["%s_%s" % (prefix, k)] for k in ("node_offsets", "children_left", "children_right", "feature", "threshold",
                                                 "missing_go_to_left", "value")}
    return audioTrainTest.ForestArrays("regressor", a["node_offsets"], a["children_left"], a["children_right"], a["feature"],
                                       a["threshold"], a["missing_go_to_left"], a["value"], None, g["vectors"].shape[0])


def _within(got, want, scale):
    err = np.abs(got - want)
    bound = 1e-9 * np.maximum(1.0, scale)
    print("max |d| %.3g, max |d| / bound %.3g" % (err.max(), (err / bound).max()))
    return np.all(err <= bound)


def _models(g):
    tasks = [str(t) for t in g["tasks"]]
    make = _forest if str(g["kind"]) == "regforest" else _svr
    return tasks, [make(g, t) for t in tasks], np.stack([g[t + "_mean"] for t in tasks]), np.stack([g[t + "_std"] for t in tasks])


def _clips(g):
    ends = np.cumsum(g["lengths"])
    return [g["signals"][e - n:e] for e, n in zip(ends, g["lengths"])]


def _windows(g):
    return float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]), float(g["st_step"]), bool(g["compute_beat"])


def test_svr_bank_matches_scikit_learn_on_the_synthetic_fits(gpu_lib):
    g = _golden("svr_synth")
    n = int(g["n_models"])
    models = [_svr(g, "m%d" % i) for i in range(n)]
    X = g["X"]
    got = audioTrainTest.regress(models, "svm", X.T, np.zeros(X.shape[1]), np.ones(X.shape[1]))
    assert got.shape == (n, X.shape[0])
    _, scale = svr_ref.bank_decision([_svr_tuple(g, "m%d" % i) for i in range(n)], X.T, np.zeros((n, X.shape[1])),
                                     np.ones((n, X.shape[1])), with_scale=True)
    assert _within(got, np.stack([g["m%d_predict" % i] for i in range(n)]), scale)
    assert np.array_equal(got[6], np.full(X.shape[0], float(g["m6_intercept"])))           # no support vectors: -rho exactly
    for i in (0, 4, 6):                                                                    # the one-vector form equals the batch
        assert audioTrainTest.regression_wrapper(models[i], "svm_rbf", X[3]) == got[i, 3]


@pytest.mark.parametrize("name", ["svr_emotion_files", "svr_linear_files"])
def test_svr_models_trained_by_the_reference(gpu_lib, name):
    g = _golden(name)
    tasks, models, means, stds = _models(g)
    got = audioTrainTest.regress(models, str(g["model_type"]), g["vectors"], means, stds)
    _, scale = svr_ref.bank_decision([_svr_tuple(g, t) for t in tasks], g["vectors"], means, stds, with_scale=True)
    assert _within(got, np.stack([g["sk_" + t] for t in tasks]), scale)
    # file_regression_signal on the clips against the reference's file_regression, by task name
    mt_win, mid_step, st_win, st_step, beat = _windows(g)
    clips = _clips(g)
    R = np.stack([audioTrainTest.file_regression_signal(c, int(g["fs"]), models, means, stds, mt_win, mid_step, st_win, st_step,
                                                        beat, str(g["model_type"])) for c in clips])
    assert _within(R.T, np.stack([g["ref_" + t] for t in tasks]), scale)


def test_forest_regressor_matches_scikit_learn_bit_for_bit(gpu_lib):
    g = _golden("regforest_emotion_files")
    tasks, models, means, stds = _models(g)
    got = audioTrainTest.regress(models, "randomforest", g["vectors"], means, stds)
    for i, t in enumerate(tasks):
        assert np.array_equal(got[i], g["sk_" + t]) and np.array_equal(got[i], g["ref_" + t])
    x = (g["vectors"][:, 1] - means[0]) / stds[0]
    assert audioTrainTest.regression_wrapper(models[0], "randomforest", x) == got[0, 1]
    assert not audioTrainTest.is_forest(models[0])
    mt_win, mid_step, st_win, st_step, beat = _windows(g)
    R = np.stack([audioTrainTest.file_regression_signal(c, int(g["fs"]), models, means, stds, mt_win, mid_step, st_win, st_step,
                                                        beat, "randomforest") for c in _clips(g)])
    # the device's long-term vectors differ from the reference's in the last bits; the SVR gate with the value's own size
    # as the scale (a forest's answer moves only when a float32 value crosses a split)
    want = np.stack([g["ref_" + t] for t in tasks])
    assert _within(R.T, want, np.abs(want))


@pytest.mark.parametrize("name", ["svr_emotion_files", "regforest_emotion_files"])
def test_batched_file_regression_equals_single_calls(gpu_lib, name):
    g = _golden(name)
    _, models, means, stds = _models(g)
    mt_win, mid_step, st_win, st_step, beat = _windows(g)
    fs, kind = int(g["fs"]), str(g["model_type"])
    clips = _clips(g)[:2]
    clips.append(clips[0][:int(0.4 * mt_win * fs)])                     # shorter than the mid-term window
    clips.append(np.zeros(int(1.5 * mt_win * fs), dtype=np.int16))     # silent
    batch = audioTrainTest.file_regression_signals(clips, fs, models, means, stds, mt_win, mid_step, st_win, st_step, beat, kind)
    assert batch.shape == (len(clips), len(models))
    for i, c in enumerate(clips):
        one = audioTrainTest.file_regression_signal(c, fs, models, means, stds, mt_win, mid_step, st_win, st_step, beat, kind)
        assert one.tobytes() == batch[i].tobytes(), i


@pytest.mark.parametrize("name", ["svr_emotion_files", "regforest_emotion_files"])
def test_mid_term_regression_equals_regress_on_the_host_matrix(gpu_lib, name):
    g = _golden(name)
    _, models, means, stds = _models(g)
    fs, kind = int(g["fs"]), str(g["model_type"])
    sig = np.concatenate(_clips(g))
    got = audioSegmentation.mid_term_regression_signal(sig, fs, models, means, stds, kind, 1.0, 0.1, 0.05, 0.05)
    mid, _, _ = MidTermFeatures.mid_feature_extraction(sig, fs, 1.0 * fs, 0.1 * fs, round(fs * 0.05), round(fs * 0.05))
    want = audioTrainTest.regress(models, kind, mid, means, stds)
    assert got.shape == (len(models), mid.shape[1]) and mid.shape[1] > 32
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("method", ["svm", "svm_rbf", "randomforest"])
def test_evaluate_regression_matches_the_restatement(gpu_lib, method):
    pytest.importorskip("sklearn")
    g = _golden("svr_evaluate")
    params = np.array([5, 10]) if method == "randomforest" else np.array([0.1, 1.0])
    np.random.seed(91)
    want, want_printed = svr_ref.evaluate_regression(g["features"], g["labels"], 5, method, params, svr_ref.sklearn_fit,
                                                     lambda m, rows: m.predict(rows))
    np.random.seed(91)
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        got = audioTrainTest.evaluate_regression(g["features"], g["labels"], 5, method, params)
    print(got, want)
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b))
    assert printed.getvalue() == want_printed


def test_trainers_report_the_device_training_error(gpu_lib):
    pytest.importorskip("sklearn")
    g = _golden("svr_evaluate")
    X, y = g["features"], g["labels"]
    for model, err in (audioTrainTest.train_svm_regression(X, y, 1.0), audioTrainTest.train_svm_regression(X, y, 1.0, kernel="rbf"),
                       audioTrainTest.train_random_forest_regression(X, y, 5)):
        want = np.mean(np.abs(model.predict(X) - y))
        assert abs(err - want) <= 1e-9 * max(1.0, want)
