"""CPU-side checks of the SVM split sweep: the NumPy restatement (tests/smo_ref.py) against live scikit-learn and against the
goldens (scripts/make_smo_golden.py), its vote rule against tests/svc_libsvm.py, and the argument errors of
paa_smo_tasks_f64 / paa_svc_fit_splits_f64, which are reported before any device work.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import smo_ref
import svc_libsvm
import train_ref
from pyaudioanalysis_amd import _ffi, audioTrainTest

KERNEL_NAMES = {0: "linear", 2: "rbf"}


def binary_cases(g):
    """[(prefix, kernel name, job, eps)] of the smo_binary golden."""
    out = []
    for c in range(int(g["n_cases"])):
        p = "c%d_" % c
        out.append((p, KERNEL_NAMES[int(g[p + "kernel_type"])],
                    (g["train_idx"], g["test_idx"], g[p + "mean"], g[p + "scale"], float(g[p + "C"])), float(g[p + "eps"])))
    return out


def sweep_jobs(g):
    """The jobs (train_idx, test_idx, mean, scale, C) of a smo_sweep golden."""
    tro, teo = g["train_off"], g["test_off"]
    return [(g["train_idx"][tro[j]:tro[j + 1]], g["test_idx"][teo[j]:teo[j + 1]], g["mean"][j], g["scale"][j], float(g["C"][j]))
            for j in range(len(tro) - 1)]


def near_rows(sk_dec, tol):
    """The test rows on which a label may differ from scikit-learn's: some pair within 2.5 tol max|dec| of zero."""
    if sk_dec.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    return np.any(np.abs(sk_dec) <= 2.5 * tol * np.max(np.abs(sk_dec)), axis=1)


@pytest.mark.parametrize("eps", [1e-3, 1e-9])
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_restatement_against_live_scikit_learn(kernel, eps):
    """Decision values within 4 x the distance the float32 kernel cache of libsvm is known to cause at this eps (the issue's
    measurements on 300 x 20 data: 2.0e-3 at 1e-3, 1.5e-5 at 1e-9), labels equal away from zero decision values."""
    sklearn_svm = pytest.importorskip("sklearn.svm")
    feats = train_ref.class_features((70, 50, 40), 12, seed=41, spread=1.4)
    X, y = train_ref.features_to_matrix(feats)
    perm = np.random.default_rng(42).permutation(X.shape[0])
    tr, te = perm[:120], perm[120:]
    mean, scale = X[tr].mean(axis=0), X[tr].std(axis=0)
    bound = 4 * (2.0e-3 if eps == 1e-3 else 1.5e-5)
    for C_param in (0.05, 1.0, 20.0):
        clf = sklearn_svm.SVC(C=C_param, kernel=kernel, probability=False, gamma="auto", tol=eps, decision_function_shape="ovo")
        clf.fit((X[tr] - mean) / scale, y[tr])
        Zq = (X[te] - mean) / scale
        want = clf.decision_function(Zq)
        pred, dec, its, status, n_sv, classes = smo_ref.fit_job(X, y, (tr, te, mean, scale, C_param), kernel, None, eps)
        assert np.all(status == smo_ref.STATUS_CONVERGED) and np.array_equal(classes, clf.classes_)
        assert np.max(np.abs(dec - want)) <= bound * np.max(np.abs(want)), (kernel, eps, C_param)
        near = near_rows(want, bound)
        assert np.array_equal(pred[~near], clf.predict(Zq)[~near])


def test_restatement_against_the_goldens():
    g = train_ref.load_golden("smo_binary")
    X, y = g["X"], g["labels"]
    for p, kernel, job, eps in binary_cases(g):
        pred, dec, its, status, n_sv, classes = smo_ref.fit_job(X, y, job, kernel, None, eps)
        tol = float(g[p + "tol_dec"])
        assert np.max(np.abs(dec[:, 0] - g[p + "sk_dec"])) <= tol * np.max(np.abs(g[p + "sk_dec"])), p
        near = near_rows(g[p + "sk_dec"].reshape(-1, 1), tol)
        assert np.count_nonzero(near) <= 0.02 * near.shape[0]
        assert np.array_equal(pred[~near], g[p + "sk_pred"][~near]), p
    for name in ("smo_sweep_linear", "smo_sweep_rbf"):
        g = train_ref.load_golden(name)
        for j, job in enumerate(sweep_jobs(g)):
            a, b = int(g["test_off"][j]), int(g["test_off"][j + 1])
            pred, dec, its, status, n_sv, classes = smo_ref.fit_job(g["X"], g["labels"], job, KERNEL_NAMES[int(g["kernel_type"])], None,
                                                                    float(g["eps"]))
            assert dec.shape == (b - a, int(g["n_pairs"][j]))
            if a == b:
                continue
            sk = g["sk_dec"][a:b, :dec.shape[1]]
            assert np.max(np.abs(dec - sk)) <= g["tol_dec"][j] * np.max(np.abs(sk)), (name, j)
            near = near_rows(sk, g["tol_dec"][j])
            assert np.count_nonzero(near) <= 0.02 * (b - a)
            assert np.array_equal(pred[~near], g["sk_pred"][a:b][~near]), (name, j)


def test_sweep_goldens_have_the_edge_jobs():
    g = train_ref.load_golden("smo_sweep_linear")
    assert g["X"].shape == (240, 20) and len(g["C"]) == 6 and len(np.unique(g["C"])) == 2
    assert sorted(g["n_pairs"].tolist()) == [1, 1, 3, 3, 3, 3]
    assert np.count_nonzero(np.diff(g["test_off"]) == 0) == 2


def test_votes_rule_is_libsvms():
    rng = np.random.default_rng(5)
    for k in (2, 3, 5, 8):
        dec = rng.standard_normal((200, k * (k - 1) // 2))
        dec[rng.random(dec.shape) < 0.1] = 0.0          # a zero decision value votes for the second class
        assert np.array_equal(smo_ref.votes_winner(dec, k), svc_libsvm.votes_winner(dec, k))


def test_solver_meets_its_own_conditions():
    """The restatement's solution satisfies the box, the equality constraint and the stopping rule recomputed from alpha."""
    rng = np.random.default_rng(6)
    Z = rng.standard_normal((90, 7))
    y = np.where(rng.random(90) < 0.5, 1.0, -1.0)
    for kernel in ("linear", "rbf"):
        K = smo_ref.gram(Z, kernel, 1.0 / 7)
        for C_param in (0.001, 1.0, 20.0):
            alpha, rho, it, gap, status = smo_ref.solve(K, y, C_param, 1e-3)
            assert status == smo_ref.STATUS_CONVERGED and np.all(alpha >= 0) and np.all(alpha <= C_param)
            assert abs(np.sum(alpha * y)) <= 4 * max(it, 1) * C_param * 2.0**-52
            G = smo_ref.gradient(K, y, alpha)
            gmax, gmax2 = smo_ref.gap_and_sets(alpha, G, y, C_param)[:2]
            assert gmax + gmax2 <= 1e-3 * (1 + 1e-6) + 1e-9 * max(1.0, np.max(np.abs(G)))
            assert abs(smo_ref.rho_of(alpha, G, y, C_param) - rho) <= 1e-9 * max(1.0, abs(rho))
    alpha, rho, it, gap, status = smo_ref.solve(smo_ref.gram(Z, "linear", 0), y, 20.0, 1e-3, max_iter=5)
    assert status == smo_ref.STATUS_NOT_CONVERGED and it == 5 and np.isfinite(rho) and gap >= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI judges its arguments before the device is initialised
# ---------------------------------------------------------------------------------------------------------------------
def _p(a, kind):
    return None if a is None else a.ctypes.data_as(kind)


class _Tasks:
    """A valid two-task call of paa_smo_tasks_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_tasks, self.kernel_type, self.eps, self.max_iter, self.ipl = 6, 3, 2, 2, 1e-3, 100, 0
        self.X = np.zeros((6, 3))
        self.task_off, self.task_idx = np.array([0, 3, 5], dtype=np.int64), np.array([0, 1, 2, 3, 4], dtype=np.int32)
        self.task_sign = np.array([1, -1, 1, 1, -1], dtype=np.int8)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.C, self.gamma = np.array([1.0, 2.0]), np.array([0.5, 0.5])
        self.alpha_y, self.rho, self.gap = np.zeros(5), np.zeros(2), np.zeros(2)
        self.iterations, self.status = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_smo_tasks_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, self.n_tasks, _p(self.task_off, _ffi.c_i64p), _p(self.task_idx, _ffi.c_i32p),
            _p(self.task_sign, C.POINTER(C.c_int8)), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), _p(self.C, _ffi.c_f64p),
            _p(self.gamma, _ffi.c_f64p), self.kernel_type, self.eps, self.max_iter, self.ipl, _p(self.alpha_y, _ffi.c_f64p),
            _p(self.rho, _ffi.c_f64p), _p(self.iterations, _ffi.c_i32p), _p(self.gap, _ffi.c_f64p), _p(self.status, _ffi.c_i32p), None)


class _Splits:
    """A valid two-job call of paa_svc_fit_splits_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.kernel_type, self.eps, self.max_iter, self.ipl = 6, 3, 2, 0, 1e-3, 100, 0
        self.X = np.zeros((6, 3))
        self.labels = np.array([0, 1, 0, 1, 2, 1], dtype=np.int32)
        self.train_off, self.train_idx = np.array([0, 3, 6], dtype=np.int64), np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)
        self.test_off, self.test_idx = np.array([0, 2, 3], dtype=np.int64), np.array([4, 5, 0], dtype=np.int32)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.C, self.gamma = np.array([1.0, 2.0]), np.array([0.5, 0.5])
        self.label_out, self.dec_out, self.max_pairs, self.n_tasks = np.zeros(3, dtype=np.int32), np.zeros((3, 1)), 1, 2
        self.task_iterations = np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_svc_fit_splits_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.labels, _ffi.c_i32p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.test_off, _ffi.c_i64p), _p(self.test_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p),
            _p(self.std, _ffi.c_f64p), _p(self.C, _ffi.c_f64p), _p(self.gamma, _ffi.c_f64p), self.kernel_type, self.eps, self.max_iter,
            self.ipl, _p(self.label_out, _ffi.c_i32p), _p(self.dec_out, _ffi.c_f64p), self.max_pairs, self.n_tasks,
            _p(self.task_iterations, _ffi.c_i32p), None, None, None)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _i64(*v):
    return np.array(v, dtype=np.int64)


def test_c_abi_rejects_bad_tasks_before_any_device_work():
    for name in ("X", "task_off", "task_idx", "task_sign", "mean", "std", "C", "gamma", "alpha_y", "rho", "iterations", "gap", "status"):
        assert _Tasks()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(task_off=_i64(1, 3, 5)), dict(task_off=_i64(0, 3, 2)), dict(task_off=_i64(0, 0, 5)), dict(task_idx=_i32(0, 1, 2, 3, 6)),
           dict(task_idx=_i32(0, -1, 2, 3, 4)), dict(task_sign=np.array([1, 0, 1, 1, -1], dtype=np.int8)), dict(n_dims=0),
           dict(C=np.array([1.0, 0.0])), dict(C=np.array([-1.0, 1.0])), dict(gamma=np.array([0.5, 0.0])), dict(eps=0.0), dict(eps=-1e-3),
           dict(kernel_type=1), dict(max_iter=0), dict(ipl=-1), dict(n_tasks=0), dict(n_samples=0), dict(n_samples=2**31)]
    for kw in bad:
        assert _Tasks()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    # beyond the limits: refused with the limit in the message, no other path
    assert _Tasks()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    geo = audioTrainTest.smo_geometry()
    assert geo == (256, 32, 8192, 32, 1024, 256)
    big = _Tasks()
    n = geo[2] + 1
    assert big(n_tasks=1, task_off=_i64(0, n), task_idx=np.zeros(n, dtype=np.int32), task_sign=np.ones(n, dtype=np.int8),
               alpha_y=np.zeros(n)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()
    assert _ffi.lib().paa_debug_smo_geometry(None) == _ffi.ERR_ARG
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "paa_hip.h")).read()
    assert "#define PAA_SMO_MAX_ROWS 8192" in header and "#define PAA_SMO_MAX_DIMS 256" in header


def test_c_abi_rejects_bad_svm_split_jobs_before_any_device_work():
    for name in ("X", "labels", "train_off", "train_idx", "test_off", "test_idx", "mean", "std", "C", "gamma", "label_out"):
        assert _Splits()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(train_off=_i64(1, 3, 6)), dict(test_off=_i64(-1, 2, 3)), dict(train_off=_i64(0, 4, 3)), dict(test_off=_i64(0, 2, 1)),
           dict(train_idx=_i32(0, 1, 2, 3, 4, 6)), dict(train_idx=_i32(0, -1, 2, 3, 4, 5)), dict(test_idx=_i32(4, 6, 0)),
           dict(n_dims=0), dict(C=np.array([1.0, 0.0])), dict(C=np.array([-2.0, 1.0])), dict(eps=0.0), dict(kernel_type=1),
           dict(kernel_type=2, gamma=np.array([0.0, 0.5])), dict(max_iter=0), dict(n_jobs=0), dict(n_samples=0),
           dict(labels=_i32(0, 0, 0, 1, 2, 1)),                                     # job 0 trains on samples 0, 1, 2: one class
           dict(labels=_i32(0, -1, 0, 1, 2, 1)),                                    # a training row without a class
           dict(train_off=_i64(0, 0, 6)),                                           # an empty training list
           dict(max_pairs=0), dict(n_tasks=3),                                      # each job makes one task: 2 in all
           dict(test_off=_i64(0, 2, 2**31))]
    for kw in bad:
        assert _Splits()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _Splits()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()


def test_python_entry_points_reject_bad_arguments():
    X = np.zeros((6, 3))
    y = np.array([0., 1, 0, 1, 0, 1])
    job = (np.array([0, 1, 2]), np.array([3, 4]), np.zeros(3), np.ones(3), 1.0)
    for args in ((np.zeros(6), y, [job]), (X, y[:5], [job]), (X, y, []), (X, y, [job[:4]]), (X, y, [(job[0], job[1], np.zeros(2), np.ones(3), 1.0)])):
        with pytest.raises(ValueError):
            audioTrainTest.svm_split_fit_predict(*args)
    with pytest.raises(NotImplementedError):
        audioTrainTest.svm_split_fit_predict(X, y, [job], kernel="poly")
    with pytest.raises(ValueError):                     # one class in the training list: the library's argument error
        audioTrainTest.svm_split_fit_predict(X, y, [(np.array([0, 2]), job[1], job[2], job[3], 1.0)])
    with pytest.raises(ValueError):
        audioTrainTest.svm_split_fit_predict(X, y, [(job[0], job[1], job[2], job[3], 0.0)])
    task = (np.array([0, 1, 2]), np.array([1, -1, 1]), np.zeros(3), np.ones(3), 1.0, None)
    for tasks in ([], [task[:5]], [(task[0], task[1][:2]) + task[2:]], [(task[0], np.array([1, 2, 1])) + task[2:]]):
        with pytest.raises(ValueError):
            audioTrainTest.smo_solve(X, tasks)
    with pytest.raises(ValueError):
        audioTrainTest.smo_solve(X, [task], eps=0.0)
    feats = train_ref.three_class_features()
    for kind in ("knn", "randomforest"):
        with pytest.raises(ValueError):
            audioTrainTest.evaluate_classifier(feats, ["a", "b", "c"], kind, [1], 0, svm_fit="device")
    with pytest.raises(ValueError):
        audioTrainTest.evaluate_classifier(feats, ["a", "b", "c"], "svm", [1], 0, svm_fit="gpu")
    with pytest.raises(ValueError):
        audioTrainTest.extract_features_and_train(["x"], 1.0, 1.0, 0.05, 0.05, "knn", "model", svm_fit="device")
    with pytest.raises(TypeError):                      # keyword only
        audioTrainTest.evaluate_classifier(feats, ["a", "b", "c"], "svm", [1], 0, None, -1, 0.9, False, "device")


def test_new_symbols_are_declared_and_built():
    from pyaudioanalysis_amd import _build
    for s in ("paa_smo_tasks_f64", "paa_svc_fit_splits_f64", "paa_debug_smo_geometry"):
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s), s
    assert "family_smo.hip" in _build.SOURCES and "family_smo.hip" not in _build.UNIT_FLAGS
