"""CPU-side checks of the probabilistic SVM fit: the fold builder and the sigmoid of the NumPy restatement (tests/platt_ref.py)
against live scikit-learn, the goldens' own conditions (scripts/make_platt_golden.py) on the restatement alone, the argument
errors of paa_platt_sigmoid_f64 / paa_svc_fit_proba_f64 and of the Python keywords, which are reported before any device work,
to_sklearn_svc, and which silence_*.npz goldens the CPU restatement of silence_removal(svm_fit="device") reproduces.  No GPU
needed."""
import ctypes as C
import glob
import os
import pickle
import re

import numpy as np
import pytest

import paa_oracle as O
import platt_ref
import train_ref
from conftest import GOLDEN_DIR
from pyaudioanalysis_amd import _build, _ffi, audioSegmentation, audioTrainTest

KERNEL_NAMES = {0: "linear", 2: "rbf"}
GOLDENS = ("platt_small", "platt_dims", "platt_big")
QUANTITIES = ("ab", "cv", "proba")


def golden_cases(name):
    """[dict] of a platt_* golden: the fields of every case, `kernel` as a name and `job` = (train_idx, mean, scale, C)."""
    g = train_ref.load_golden(name)
    cases = []
    for i in range(int(g["n_cases"])):
        p = "c%d_" % i
        c = {k[len(p):]: v for k, v in g.items() if k.startswith(p)}
        c["name"] = "%s_%s" % (str(c["name"]), KERNEL_NAMES[int(c["kernel_type"])])
        c["kernel"] = KERNEL_NAMES[int(c["kernel_type"])]
        c["job"] = (c["train_idx"], c["mean"], c["scale"], float(c["C"]))
        cases.append(c)
    return cases


def dense_coef(model, n_train):
    """_dual_coef_ [k - 1][n_SV] scattered to the training rows."""
    coef = np.zeros((np.asarray(model._dual_coef_).shape[0], n_train))
    coef[:, np.asarray(model.support_)] = model._dual_coef_
    return coef


def distances(c, ab, cv, coef, intercept, proba):
    """The distances of a fit to scikit-learn's answers in the golden case c, as scripts/make_platt_golden.py measures them
    (coef: the coefficients over C and the intercepts over max(1, |intercept|), for the reader: it carries no tolerance)."""
    sk_ab = np.stack([c["sk_probA"], c["sk_probB"]], axis=1)
    return {"ab": float(np.max(np.abs(ab - sk_ab) / np.maximum(1.0, np.max(np.abs(sk_ab), axis=1, keepdims=True)))),
            "cv": float(np.max(np.abs(cv - c["sk_cv_dec"])) / np.max(np.abs(c["sk_cv_dec"]))),
            "coef": float(max(np.max(np.abs(coef - c["sk_coef"])) / float(c["C"]),
                              np.max(np.abs(intercept - c["sk_intercept"]) / np.maximum(1.0, np.abs(c["sk_intercept"]))))),
            "proba": float(np.max(np.abs(proba - c["sk_proba"])))}


# ---------------------------------------------------------------------------------------------------------------------
# the seed rule, the folds and the sigmoid against scikit-learn
# ---------------------------------------------------------------------------------------------------------------------
def test_generator_is_std_mt19937():
    assert platt_ref._Mt(5489).raw() == 3499211612          # the first output of a default-constructed std::mt19937
    assert sorted(platt_ref.permutation(13, 4).tolist()) == list(range(13))


@pytest.mark.parametrize("case", golden_cases("platt_small"), ids=lambda c: c["name"])
def test_fold_builder_and_sigmoid_against_live_scikit_learn(case):
    """scikit-learn's own probability=False fits on the restatement's folds, then the restatement's sigmoid_train, give probA_ /
    probB_ of SVC(probability=True, random_state=r) within 1e-9: the seed rule, the permutation, the folds, the degenerate
    constants and the orientation are libsvm's."""
    sklearn_svm = pytest.importorskip("sklearn.svm")
    c = case
    X, lab, kernel, r = c["X"], c["labels"], c["kernel"], int(c["random_state"])
    Z = (X[c["train_idx"]] - c["mean"]) / c["scale"]
    sk = sklearn_svm.SVC(C=float(c["C"]), kernel=kernel, probability=True, gamma="auto", random_state=r).fit(Z, lab[c["train_idx"]])
    seed = int(np.random.RandomState(r).randint(np.iinfo('i').max))
    assert seed == int(c["seed"])

    def fold_dec(Zt, y, C_, Zh):
        m = sklearn_svm.SVC(C=C_, kernel=kernel, gamma=1.0 / X.shape[1]).fit(Zt, y)
        return m.decision_function(Zh) * (1.0 if m.classes_[1] == 1 else -1.0)

    _, pairs = platt_ref.fit(X, lab, c["job"], seed, kernel, fold_dec=fold_dec)
    ab = np.array([[q["prob_a"], q["prob_b"]] for q in pairs])
    assert np.max(np.abs(ab - np.stack([sk.probA_, sk.probB_], axis=1))) <= 1e-9
    assert np.max(np.abs(np.concatenate([q["cv_dec"] for q in pairs]) - c["sk_cv_dec"])) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# the goldens' own conditions, on the restatement alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_meet_their_own_conditions(name):
    pytest.importorskip("sklearn.svm")                      # (the restatement's probabilities go through to_sklearn_svc)
    cases = golden_cases(name)
    for c in cases:
        for q in QUANTITIES:                                # the stored rule: 4 x the measured distance, at least 1e-9
            assert float(c["tol_" + q]) == max(4.0 * float(c["dist_" + q]), 1e-9), (c["name"], q)
        classes, pairs = platt_ref.fit(c["X"], c["labels"], c["job"], int(c["seed"]), c["kernel"])
        assert all(q["sigmoid_stop"] == platt_ref.STOP_CONVERGED for q in pairs)
        model = platt_ref.model_of(c["X"], c["labels"], c["job"], classes, pairs, c["kernel"])
        Zq = (c["X"][c["test_idx"]] - c["mean"]) / c["scale"]
        got = distances(c, np.array([[q["prob_a"], q["prob_b"]] for q in pairs]), np.concatenate([q["cv_dec"] for q in pairs]),
                        dense_coef(model, len(c["train_idx"])), model._intercept_, audioTrainTest.to_sklearn_svc(model).predict_proba(Zq))
        for q in QUANTITIES:                                # the restatement is where the golden says it is
            assert got[q] <= float(c["dist_" + q]) * (1 + 1e-6) + 1e-12, (c["name"], q, got[q])
        degenerate = np.concatenate([q["degenerate"] for q in pairs])
        assert np.array_equal(degenerate, c["degenerate"])
        assert np.all(np.isin(c["sk_cv_dec"][degenerate], (-1.0, 0.0, 1.0)))
    by_name = {c["name"]: c for c in cases}
    if name == "platt_small":
        assert np.count_nonzero(by_name["degenerate_13_2_linear"]["degenerate"]) >= 1
        folds = platt_ref.pair_folds(np.array([1.0, 1.0, -1.0, -1.0]), int(by_name["l4_linear"]["seed"]))
        assert [len(held) for held, _, _ in folds] == [0, 1, 1, 1, 1]           # l = 4: the first fold is empty
        assert np.bincount(by_name["three_classes_rbf"]["labels"][by_name["three_classes_rbf"]["train_idx"]]).tolist() == [25, 14, 3]
    if name == "platt_dims":
        assert sorted({c["X"].shape[1] for c in cases}) == [1, 8, 9, 68, 136, 256]
    if name == "platt_big":
        T, _, _, per_block = audioTrainTest.smo_geometry()[:4]
        assert len(by_name["big_pair_linear"]["train_idx"]) > max(T, 16 * 5, per_block * 5)      # every fold: several tiles and steps
        a, b = by_name["two_jobs_0_linear"], by_name["two_jobs_1_linear"]
        assert np.array_equal(a["X"], b["X"]) and float(a["C"]) != float(b["C"]) and int(a["seed"]) != int(b["seed"])


def test_degenerate_constants_follow_the_training_part():
    signs = np.array([1.0] * 5 + [-1.0])
    seen = set()
    for seed in range(40):
        for held, train, constant in platt_ref.pair_folds(signs, seed):
            rest = np.setdiff1d(np.arange(6), held)
            if train is None:
                assert np.all(signs[rest] == constant) and constant in (1.0, -1.0)
                seen.add(constant)
            else:
                assert sorted(train.tolist()) == rest.tolist() and signs[train[0]] != signs[train[-1]]
    assert seen == {1.0}
    # l = 1: four empty folds, and the fold that holds the row out trains on nothing
    assert [(len(h), tr, c) for h, tr, c in platt_ref.pair_folds(np.array([1.0]), 3)] == [(0, None, 1.0)] * 4 + [(1, None, 0.0)]


def test_sigmoid_restatement_on_a_known_answer():
    """Symmetric data: B = 0 by symmetry and A solves the one-dimensional stationarity condition."""
    dec = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 0.3, -0.3])
    signs = np.array([-1, -1, -1, 1, 1, 1, -1, 1])
    A, B, it, stop, margin = platt_ref.sigmoid_train(dec, signs)
    assert stop == platt_ref.STOP_CONVERGED and 0 < it < 20 and margin > 0
    t = np.where(signs > 0, 5.0 / 6.0, 1.0 / 6.0)
    p = 1.0 / (1.0 + np.exp(A * dec + B))
    assert abs(B) < 1e-9 and abs(np.sum(dec * (t - p))) < 1e-5 and A < 0


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI and the Python layer judge their arguments before the device is initialised
# ---------------------------------------------------------------------------------------------------------------------
def _p(a, kind):
    return None if a is None else a.ctypes.data_as(kind)


class _Sigmoid:
    """A valid two-problem call of paa_platt_sigmoid_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.dec, self.sign = np.array([0.5, -0.5, 1.0, 0.2, -0.1]), np.array([1, -1, 1, 1, -1], dtype=np.int8)
        self.n, self.off = 2, np.array([0, 3, 5], dtype=np.int64)
        self.A, self.B, self.it, self.stop = np.zeros(2), np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_platt_sigmoid_f64(_p(self.dec, _ffi.c_f64p), _p(self.sign, C.POINTER(C.c_int8)), self.n, _p(self.off, _ffi.c_i64p),
                                                _p(self.A, _ffi.c_f64p), _p(self.B, _ffi.c_f64p), _p(self.it, _ffi.c_i32p),
                                                _p(self.stop, _ffi.c_i32p))


class _Proba:
    """A valid one-job call of paa_svc_fit_proba_f64 (two classes of 3 + 2 rows) whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.kernel_type, self.eps, self.max_iter, self.ipl = 6, 3, 1, 2, 1e-3, 100, 0
        self.X, self.labels = np.zeros((6, 3)), np.array([0, 1, 0, 1, 0, 5], dtype=np.int32)
        self.train_off, self.train_idx = np.array([0, 5], dtype=np.int64), np.array([0, 1, 2, 3, 4], dtype=np.int32)
        self.mean, self.std, self.C, self.gamma = np.zeros((1, 3)), np.ones((1, 3)), np.array([1.0]), np.array([0.5])
        self.seed, self.n_pairs, self.n_rows = np.array([7], dtype=np.int64), 1, 5
        self.alpha_y, self.rho, self.prob_a, self.prob_b = np.zeros(5), np.zeros(1), np.zeros(1), np.zeros(1)
        self.n_sv, self.sig_it, self.sig_stop = (np.zeros(1, dtype=np.int32) for _ in range(3))
        self.task_it, self.task_status = np.zeros((1, 6), dtype=np.int32), np.zeros((1, 6), dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_svc_fit_proba_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.labels, _ffi.c_i32p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), _p(self.C, _ffi.c_f64p),
            _p(self.gamma, _ffi.c_f64p), self.kernel_type, self.eps, self.max_iter, self.ipl, _p(self.seed, _ffi.c_i64p), self.n_pairs,
            self.n_rows, _p(self.alpha_y, _ffi.c_f64p), _p(self.rho, _ffi.c_f64p), _p(self.prob_a, _ffi.c_f64p), _p(self.prob_b, _ffi.c_f64p),
            _p(self.n_sv, _ffi.c_i32p), _p(self.task_it, _ffi.c_i32p), _p(self.task_status, _ffi.c_i32p), _p(self.sig_it, _ffi.c_i32p),
            _p(self.sig_stop, _ffi.c_i32p), None, None)


def test_c_abi_rejects_bad_sigmoid_problems_before_any_device_work():
    for name in ("dec", "sign", "off", "A", "B", "it", "stop"):
        assert _Sigmoid()(**{name: None}) == _ffi.ERR_ARG, name
    for kw in (dict(n=0), dict(off=np.array([1, 3, 5], dtype=np.int64)), dict(off=np.array([0, 3, 2], dtype=np.int64)),
               dict(off=np.array([0, 0, 5], dtype=np.int64)), dict(sign=np.array([1, -1, 0, 1, -1], dtype=np.int8)),
               dict(sign=np.array([1, -1, 2, 1, -1], dtype=np.int8))):
        assert _Sigmoid()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    n = 8193
    assert _Sigmoid()(n=1, off=np.array([0, n], dtype=np.int64), dec=np.zeros(n), sign=np.ones(n, dtype=np.int8)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()


def test_c_abi_rejects_bad_proba_jobs_before_any_device_work():
    for name in ("X", "labels", "train_off", "train_idx", "mean", "std", "C", "gamma", "seed", "alpha_y", "rho", "prob_a", "prob_b", "n_sv",
                 "task_it", "task_status", "sig_it", "sig_stop"):
        assert _Proba()(**{name: None}) == _ffi.ERR_ARG, name
    for kw in (dict(seed=np.array([-1], dtype=np.int64)), dict(seed=np.array([2**31], dtype=np.int64)), dict(n_pairs=2), dict(n_rows=4),
               dict(n_jobs=0), dict(n_dims=0), dict(kernel_type=1), dict(eps=0.0), dict(max_iter=0), dict(ipl=-1),
               dict(C=np.array([0.0])), dict(gamma=np.array([0.0])), dict(train_idx=np.array([0, 1, 2, 3, 6], dtype=np.int32)),
               dict(train_off=np.array([1, 5], dtype=np.int64)), dict(labels=np.array([0, -1, 0, 1, 0, 5], dtype=np.int32)),
               dict(labels=np.zeros(6, dtype=np.int32))):                # one class: an SVM needs two
        assert _Proba()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert "seed" in (_Proba()(seed=np.array([-1], dtype=np.int64)), _ffi.last_error())[1]
    assert _Proba()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = 8193
    big = dict(n_samples=n, X=np.zeros((n, 3)), labels=(np.arange(n) % 2).astype(np.int32), train_off=np.array([0, n], dtype=np.int64),
               train_idx=np.arange(n, dtype=np.int32), n_rows=n, alpha_y=np.zeros(n))
    assert _Proba()(**big) == _ffi.ERR_UNSUPPORTED and "8192" in _ffi.last_error()


def test_python_entry_points_reject_bad_arguments():
    X, y = np.zeros((6, 3)), np.array([0, 1, 0, 1, 0, 1])
    job = (np.arange(6), np.zeros(3), np.ones(3), 1.0)
    with pytest.raises(ValueError):                     # seed < 0
        audioTrainTest.svc_fit_proba(X, y, [job], seeds=-1)
    with pytest.raises(ValueError):
        audioTrainTest.svc_fit_proba(X, y, [job, job], seeds=[1, 2, 3])
    with pytest.raises(ValueError):                     # the split sweep's job form has five fields
        audioTrainTest.svc_fit_proba(X, y, [(np.arange(6), np.arange(0), np.zeros(3), np.ones(3), 1.0)])
    with pytest.raises(ValueError):
        audioTrainTest.svc_fit_proba(X, y, [])
    with pytest.raises(NotImplementedError):
        audioTrainTest.svc_fit_proba(X, y, [job], kernel="poly")
    with pytest.raises(ValueError):                     # one class: the library's argument error
        audioTrainTest.svc_fit_proba(X, np.zeros(6), [job])
    with pytest.raises(ValueError):
        audioTrainTest.platt_sigmoid([0.1, 0.2], [1, -1, 1], [0, 2])
    with pytest.raises(ValueError):
        audioTrainTest.platt_sigmoid([0.1, 0.2], [1, 0], [0, 2])
    with pytest.raises(ValueError):
        audioTrainTest.platt_sigmoid([0.1, 0.2], [1, -1], [0, 3])
    with pytest.raises(NotImplementedError, match="8192"):          # a pair above 8192 rows, no CPU fallback
        audioTrainTest.train_svm_device(np.zeros((8193, 2)), np.arange(8193) % 2, 1.0)
    with pytest.raises(ValueError):
        audioTrainTest.train_svm_device(np.zeros((5, 2)), np.zeros(5), 1.0)
    with pytest.raises(TypeError):                      # keyword only
        audioTrainTest.train_svm_device(np.zeros((6, 2)), y, 1.0, "linear", 3)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):                     # svm_fit="gpu" on silence_removal, before any work
        audioSegmentation.silence_removal(np.zeros(16000), 16000, 0.05, 0.05, svm_fit="gpu")
    with pytest.raises(TypeError):
        audioSegmentation.silence_removal(np.zeros(16000), 16000, 0.05, 0.05, 0.5, 0.5, False, "device")
    with pytest.raises(ValueError):                     # final_fit="device" serves the SVM types only, refused before any work
        audioTrainTest.extract_features_and_train(["x"], 1.0, 1.0, 0.05, 0.05, "knn", "model", final_fit="device")
    with pytest.raises(ValueError):
        audioTrainTest.extract_features_and_train(["x"], 1.0, 1.0, 0.05, 0.05, "svm", "model", final_fit="gpu")
    assert np.array_equal(np.random.get_state()[1], state)


def test_libsvm_seed_is_scikit_learns_draw():
    np.random.seed(5)
    want = np.random.randint(np.iinfo('i').max)
    after = np.random.get_state()[1].copy()
    np.random.seed(5)
    assert audioTrainTest._libsvm_seed(None) == want and np.array_equal(np.random.get_state()[1], after)     # one draw, the same
    assert audioTrainTest._libsvm_seed(11) == np.random.RandomState(11).randint(np.iinfo('i').max)
    assert audioTrainTest._libsvm_seed(np.random.RandomState(11)) == audioTrainTest._libsvm_seed(11)


def test_new_symbols_are_declared_bound_and_built():
    header = open(os.path.join(os.path.dirname(_build.CSRC), "..", "include", "paa_hip.h")).read()
    for s in ("paa_platt_sigmoid_f64", "paa_svc_fit_proba_f64"):
        assert re.search(r"^int %s\(" % s, header, re.M), s
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s), s
    assert "Not served: Platt probabilities" not in header
    assert "kernels_platt.hpp" in _build.HEADERS and len(_build.SOURCES) == 18
    assert '#include "kernels_platt.hpp"' in open(os.path.join(_build.CSRC, "family_smo.hip")).read()


# ---------------------------------------------------------------------------------------------------------------------
# to_sklearn_svc
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,kernel", [((30, 25), "linear"), ((30, 25), "rbf"), ((25, 14, 9), "linear"), ((25, 14, 9), "rbf")])
def test_to_sklearn_svc_predicts_as_the_fit_it_was_filled_from(sizes, kernel):
    sklearn_svm = pytest.importorskip("sklearn.svm")
    rng = np.random.RandomState(len(sizes))
    y = np.concatenate([np.full(n, 10 * c) for c, n in enumerate(sizes)])
    X = rng.randn(len(y), 5) + 0.1 * y[:, None]
    order = rng.permutation(len(y))
    X, y = X[order], y[order]
    sk = sklearn_svm.SVC(C=2.0, kernel=kernel, probability=True, gamma="auto", random_state=1).fit(X, y)
    stand_in = platt_ref.Model(support_=sk.support_, support_vectors_=sk.support_vectors_, n_support_=sk.n_support_, _dual_coef_=sk._dual_coef_,
                               _intercept_=sk._intercept_, probA_=sk.probA_, probB_=sk.probB_, classes_=sk.classes_, kernel=kernel,
                               _gamma=sk._gamma, C=2.0, shape_fit_=sk.shape_fit_)
    Xq = rng.randn(40, 5) + 10.0 * rng.randint(0, len(sizes), 40)[:, None] * 0.1
    for svc in (audioTrainTest.to_sklearn_svc(stand_in), pickle.loads(pickle.dumps(audioTrainTest.to_sklearn_svc(stand_in)))):
        assert isinstance(svc, sklearn_svm.SVC)
        assert np.array_equal(svc.predict(Xq), sk.predict(Xq))
        assert svc.predict_proba(Xq).tobytes() == sk.predict_proba(Xq).tobytes()
        assert svc.decision_function(Xq).tobytes() == sk.decision_function(Xq).tobytes()
        assert np.array_equal(svc.dual_coef_, sk.dual_coef_) and np.array_equal(svc.intercept_, sk.intercept_)
        assert np.array_equal(svc.n_support_, sk.n_support_)


# ---------------------------------------------------------------------------------------------------------------------
# silence_removal(svm_fit="device") restated on the CPU: which goldens it reproduces
# ---------------------------------------------------------------------------------------------------------------------
SILENCE_GOLDENS = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "silence_*.npz")))
# the goldens whose segments the CPU restatement reproduces at atol 1e-9: the GPU test holds the device mode to these
SILENCE_REPRODUCED = tuple(SILENCE_GOLDENS)


def cpu_train_svm_device(features, labels, c_param, kernel, random_state, mean, scale):
    """audioTrainTest._train_svm_device on the CPU: the restatement's fits for scikit-learn's draw of the seed."""
    seed = audioTrainTest._libsvm_seed(random_state)
    X = np.asarray(features, dtype=np.float64)
    job = (np.arange(X.shape[0]), mean, scale, float(c_param))
    classes, pairs = platt_ref.fit(X, labels, job, seed, kernel)
    return platt_ref.model_of(X, labels, job, classes, pairs, kernel)


@pytest.mark.parametrize("name", SILENCE_GOLDENS)
def test_silence_removal_device_mode_restated_on_the_cpu(monkeypatch, name):
    pytest.importorskip("sklearn.svm")
    g = train_ref.load_golden(name)
    from pyaudioanalysis_amd import ShortTermFeatures as product_stf
    monkeypatch.setattr(product_stf, "feature_extraction",
                        lambda sig, rate, win, step, deltas=True: O.feature_extraction(sig, rate, win, step, deltas))
    monkeypatch.setattr(audioTrainTest, "_train_svm_device", cpu_train_svm_device)

    def predict_all(st_feats, mean, std, svm):
        return audioTrainTest.to_sklearn_svc(svm).predict_proba(((st_feats.T - mean) / std))[:, 1]
    monkeypatch.setattr(audioSegmentation, "svm_onset_probability", predict_all)
    np.random.seed(int(g["seed"]))
    got = audioSegmentation.silence_removal(g["signal"], int(g["fs"]), float(g["st_win"]), float(g["st_step"]), float(g["smooth_window"]),
                                            float(g["weight"]), svm_fit="device")
    got = np.array(got, dtype=np.float64).reshape(-1, 2)
    reproduced = got.shape == g["segments"].shape and np.allclose(got, g["segments"], rtol=0, atol=1e-9)
    assert reproduced == (name in SILENCE_REPRODUCED), (name, got, g["segments"])


def test_enough_silence_goldens_remain():
    assert len(SILENCE_GOLDENS) == 4 and len(SILENCE_REPRODUCED) >= 3
