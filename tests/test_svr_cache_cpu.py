"""CPU-side checks of the SVR solver's resident kernel matrix (DESIGN K22): the argument errors of paa_svr_tasks_cached_f64,
paa_svr_fit_splits_cached_f64 and paa_svr_gram_f64, which are reported before any device work; the packing rule against a hand
count; the derivation of the Gram kernel's bounds on the exact restatement of tests/svr_cache_cases.py; the goldens' rule of the
final fit on the restatement; the Python entry points' own errors.  No GPU needed."""
import fractions
import inspect
import os

import numpy as np
import pytest

import svr_cache_cases as cases
from pyaudioanalysis_amd import _ffi, audioTrainTest
from test_svr_fit_cpu import _f64, _i32, _i64, _p, _Splits, _Tasks, small_task

NEW_SYMBOLS = ("paa_svr_tasks_cached_f64", "paa_svr_fit_splits_cached_f64", "paa_svr_gram_f64")


class _TasksCached(_Tasks):
    """A valid two-task call of paa_svr_tasks_cached_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        super().__init__()
        self.cache_bytes, self.cached = 1 << 20, np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        f, i32, i64 = _ffi.c_f64p, _ffi.c_i32p, _ffi.c_i64p
        return _ffi.lib().paa_svr_tasks_cached_f64(
            _p(self.X, f), self.n_samples, self.n_dims, _p(self.y, f), self.n_tasks, _p(self.task_off, i64), _p(self.task_idx, i32),
            _p(self.mean, f), _p(self.std, f), _p(self.C, f), _p(self.gamma, f), _p(self.epsilon, f), self.kernel_type, self.eps,
            self.max_iter, self.ipl, _p(self.beta, f), _p(self.rho, f), _p(self.iterations, i32), _p(self.gap, f), _p(self.status, i32),
            _p(self.n_sv, i32), _p(self.train_pred, f), None, self.cache_bytes, _p(self.cached, i32))


class _SplitsCached(_Splits):
    """Likewise for paa_svr_fit_splits_cached_f64."""

    def __init__(self):
        super().__init__()
        self.cache_bytes, self.cached = 1 << 20, np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        f, i32, i64 = _ffi.c_f64p, _ffi.c_i32p, _ffi.c_i64p
        return _ffi.lib().paa_svr_fit_splits_cached_f64(
            _p(self.X, f), self.n_samples, self.n_dims, _p(self.y, f), self.n_jobs, _p(self.train_off, i64), _p(self.train_idx, i32),
            _p(self.test_off, i64), _p(self.test_idx, i32), _p(self.mean, f), _p(self.std, f), _p(self.C, f), _p(self.gamma, f),
            _p(self.epsilon, f), self.kernel_type, self.eps, self.max_iter, self.ipl, _p(self.pred_out, f), _p(self.train_pred_out, f),
            None, None, None, None, self.cache_bytes, _p(self.cached, i32))


class _Gram:
    """A valid two-task call of paa_svr_gram_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_tasks, self.kernel_type = 6, 3, 2, 2
        self.X = np.zeros((6, 3))
        self.task_off, self.task_idx = np.array([0, 3, 5], dtype=np.int64), np.array([0, 1, 2, 3, 4], dtype=np.int32)
        self.mean, self.std, self.gamma = np.zeros((2, 3)), np.ones((2, 3)), np.array([0.5, 0.5])
        self.K_out, self.qd_out = np.zeros(9 + 4), np.zeros(5)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        f, i32, i64 = _ffi.c_f64p, _ffi.c_i32p, _ffi.c_i64p
        return _ffi.lib().paa_svr_gram_f64(_p(self.X, f), self.n_samples, self.n_dims, self.n_tasks, _p(self.task_off, i64),
                                           _p(self.task_idx, i32), _p(self.mean, f), _p(self.std, f), _p(self.gamma, f), self.kernel_type,
                                           _p(self.K_out, f), _p(self.qd_out, f))


def test_cached_tasks_reject_bad_arguments_before_any_device_work():
    for name in ("X", "y", "task_off", "task_idx", "mean", "std", "C", "gamma", "epsilon", "beta", "rho", "iterations", "gap", "status", "n_sv",
                 "train_pred", "cached"):
        assert _TasksCached()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(task_off=_i64(1, 3, 5)), dict(task_off=_i64(0, 3, 2)), dict(task_off=_i64(0, 0, 5)), dict(task_idx=_i32(0, 1, 2, 3, 6)),
           dict(task_idx=_i32(0, -1, 2, 3, 4)), dict(n_dims=0), dict(C=_f64(1.0, 0.0)), dict(C=_f64(-1.0, 1.0)), dict(C=_f64(np.inf, 1.0)),
           dict(gamma=_f64(0.5, 0.0)), dict(gamma=_f64(-0.5, 0.5)), dict(epsilon=_f64(-0.1, 0.1)), dict(epsilon=_f64(0.1, np.nan)),
           dict(epsilon=_f64(np.inf, 0.1)), dict(y=_f64(0, 1, np.nan, 3, 4, 5)), dict(y=_f64(0, 1, 2, 3, 4, np.inf)), dict(eps=0.0),
           dict(eps=-1e-3), dict(kernel_type=1), dict(max_iter=0), dict(ipl=-1), dict(n_tasks=0), dict(n_samples=0), dict(n_samples=2**31),
           dict(cache_bytes=0), dict(cache_bytes=-1), dict(cache_bytes=-2**40)]
    for kw in bad:
        assert _TasksCached()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _TasksCached()(cache_bytes=0) == _ffi.ERR_ARG and "cache_bytes" in _ffi.last_error()
    # the parent's arguments are judged first, in the parent's order
    assert _TasksCached()(cache_bytes=0, eps=0.0) == _ffi.ERR_ARG and "eps" in _ffi.last_error()
    assert _TasksCached()(cache_bytes=0, y=_f64(0, 1, np.nan, 3, 4, 5)) == _ffi.ERR_ARG and "target" in _ffi.last_error()
    assert _TasksCached()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = audioTrainTest.smo_geometry()[2] + 1
    assert _TasksCached()(n_tasks=1, task_off=_i64(0, n), task_idx=np.zeros(n, dtype=np.int32), beta=np.zeros(n),
                          train_pred=np.zeros(n)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()
    # a valid call reaches the device: without one it is refused there, with the "no device" error, and never computed on the CPU
    if _ffi.device_count() < 1:
        assert _TasksCached()() not in (_ffi.PAA_OK, _ffi.ERR_ARG, _ffi.ERR_UNSUPPORTED)


def test_cached_splits_reject_bad_arguments_before_any_device_work():
    for name in ("X", "y", "train_off", "train_idx", "test_off", "test_idx", "mean", "std", "C", "gamma", "epsilon", "pred_out", "cached"):
        assert _SplitsCached()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(train_off=_i64(1, 3, 6)), dict(test_off=_i64(-1, 2, 3)), dict(train_off=_i64(0, 4, 3)), dict(test_off=_i64(0, 2, 1)),
           dict(train_idx=_i32(0, 1, 2, 3, 4, 6)), dict(train_idx=_i32(0, -1, 2, 3, 4, 5)), dict(test_idx=_i32(4, 6, 0)),
           dict(n_dims=0), dict(C=_f64(1.0, 0.0)), dict(C=_f64(-2.0, 1.0)), dict(eps=0.0), dict(kernel_type=1),
           dict(kernel_type=2, gamma=_f64(0.0, 0.5)), dict(epsilon=_f64(0.1, -1e-9)), dict(epsilon=_f64(np.nan, 0.1)),
           dict(y=_f64(0, 1, 2, -np.inf, 4, 5)), dict(y=_f64(np.nan, 1, 2, 3, 4, 5)), dict(max_iter=0), dict(ipl=-1), dict(n_jobs=0),
           dict(n_samples=0), dict(train_off=_i64(0, 0, 6)), dict(test_off=_i64(0, 2, 2**31)),
           dict(cache_bytes=0), dict(cache_bytes=-8)]
    for kw in bad:
        assert _SplitsCached()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _SplitsCached()(cache_bytes=0, max_iter=0) == _ffi.ERR_ARG and "max_iter" in _ffi.last_error()
    assert _SplitsCached()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = audioTrainTest.smo_geometry()[2] + 1
    assert _SplitsCached()(n_jobs=1, train_off=_i64(0, n), test_off=_i64(0, 1), train_idx=np.zeros(n, dtype=np.int32),
                           train_pred_out=None) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()


def test_gram_entry_rejects_bad_arguments_before_any_device_work():
    for name in ("X", "task_off", "task_idx", "mean", "std", "gamma", "K_out"):
        assert _Gram()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(task_off=_i64(1, 3, 5)), dict(task_off=_i64(0, 3, 2)), dict(task_off=_i64(0, 0, 5)), dict(task_idx=_i32(0, 1, 2, 3, 6)),
           dict(task_idx=_i32(0, -1, 2, 3, 4)), dict(n_dims=0), dict(gamma=_f64(0.5, 0.0)), dict(gamma=_f64(np.nan, 0.5)), dict(kernel_type=1),
           dict(n_tasks=0), dict(n_samples=0), dict(n_samples=2**31)]
    for kw in bad:
        assert _Gram()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _Gram()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = audioTrainTest.smo_geometry()[2] + 1
    assert _Gram()(n_tasks=1, task_off=_i64(0, n), task_idx=np.zeros(n, dtype=np.int32)) == _ffi.ERR_UNSUPPORTED and "8192" in _ffi.last_error()
    assert _Gram()(kernel_type=0, gamma=_f64(0.0, 0.0), n_dims=257) == _ffi.ERR_UNSUPPORTED       # a linear kernel reads no gamma


def test_new_symbols_are_declared_exported_and_in_the_header():
    import conftest
    from pyaudioanalysis_amd import _build
    header = open(os.path.join(conftest.ROOT, "include", "paa_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s) and "int %s(" % s in header, s
    assert "kernels_svrcache.hpp" in _build.HEADERS and len(_build.SOURCES) == 18           # the unit count stays
    src = open(os.path.join(conftest.ROOT, "pyaudioanalysis_amd", "csrc", "family_svr.hip")).read()
    assert '#include "kernels_svrcache.hpp"' in src


def test_python_entry_points_reject_bad_arguments():
    aT = audioTrainTest
    X, y = np.zeros((6, 3)), np.arange(6.0)
    task = (np.array([0, 1, 2]), np.zeros(3), np.ones(3), 1.0, None, 0.1)
    job = (np.array([0, 1, 2]), np.array([3, 4]), np.zeros(3), np.ones(3), 1.0)
    for kw in (dict(kernel_cache="lru"), dict(kernel_cache="gram", cache_bytes=0), dict(kernel_cache="gram", cache_bytes=-5)):
        with pytest.raises(ValueError):
            aT.svr_solve(X, y, [task], **kw)
        with pytest.raises(ValueError):
            aT.svr_split_fit_predict(X, y, [job], **kw)
        with pytest.raises(ValueError):
            aT.evaluate_regression(*small_task(), 2, "svm", [1.0], svm_fit="device", **kw)
    for fn, names in ((aT.svr_solve, ("kernel_cache", "cache_bytes")), (aT.svr_split_fit_predict, ("kernel_cache", "cache_bytes")),
                      (aT.evaluate_regression, ("kernel_cache", "cache_bytes")), (aT.train_svm_regression_device, ("kernel_cache",)),
                      (aT.feature_extraction_train_regression, ("final_fit", "kernel_cache"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, name)
    assert inspect.signature(aT.svr_solve).parameters["kernel_cache"].default == "none"
    assert inspect.signature(aT.svr_split_fit_predict).parameters["kernel_cache"].default == "none"
    assert inspect.signature(aT.evaluate_regression).parameters["kernel_cache"].default == "none"
    assert inspect.signature(aT.feature_extraction_train_regression).parameters["final_fit"].default == "sklearn"
    assert inspect.signature(aT.train_svm_regression_device).parameters["kernel_cache"].default == "gram"
    # final_fit: "device" serves the SVR types alone
    for model_type in ("randomforest", "knn"):
        with pytest.raises(ValueError, match="final_fit"):
            aT.feature_extraction_train_regression("/nonexistent", 1.0, 1.0, 0.05, 0.05, model_type, "m", final_fit="device")
    with pytest.raises(ValueError, match="final_fit"):
        aT.feature_extraction_train_regression("/nonexistent", 1.0, 1.0, 0.05, 0.05, "svm", "m", final_fit="gpu")
    # more than 8192 rows: refused before the library is asked
    big = np.zeros((cases.MAX_ROWS + 1, 2))
    with pytest.raises(NotImplementedError, match="8192"):
        aT.train_svm_regression_device(big, np.zeros(cases.MAX_ROWS + 1), 1.0, "rbf")
    with pytest.raises(NotImplementedError):
        aT.train_svm_regression_device(X, y, 1.0, "poly")
    with pytest.raises(ValueError):
        aT.train_svm_regression_device(X, y[:5], 1.0)
    for tasks in ([], [task[:3]]):
        with pytest.raises(ValueError):
            aT.svr_kernel_matrix(X, tasks, "rbf")
    with pytest.raises(NotImplementedError):
        aT.svr_kernel_matrix(X, [task[:3] + (None,)], "poly")


def test_packing_rule_against_a_hand_count():
    for rows, budget, want in cases.PACKING_BY_HAND:
        got = audioTrainTest.svr_cache_chunks(rows, budget)
        assert got.tolist() == list(want), (rows, budget, got)
        assert np.array_equal(got >= 0, cases.expected_cached(rows, budget))
        for ch in range(got.max() + 1):                 # no chunk above the budget, chunks in task order
            assert sum(cases.matrix_bytes(n) for n, c in zip(rows, got) if c == ch) <= budget
        kept = got[got >= 0]
        assert np.all(np.diff(kept) >= 0) and (kept.size == 0 or kept[0] == 0)
    assert audioTrainTest.SVR_CACHE_BYTES == 4 << 30 and cases.matrix_bytes(8192) == 512 << 20


def test_exact_gram_is_exact():
    """The integer Gram matrix against Python fractions, on rows whose exponents spread over 40 binades."""
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((5, 11)) * 2.0 ** rng.integers(-20, 20, (5, 11))
    Z[0, 3] = 0.0
    G, A, k = cases.exact_gram(Z)
    F = [[fractions.Fraction(float(v)) for v in row] for row in Z]
    for a in range(5):
        for b in range(5):
            assert fractions.Fraction(int(G[a, b]), 1 << (2 * k)) == sum(x * y for x, y in zip(F[a], F[b]))
            assert fractions.Fraction(int(A[a, b]), 1 << (2 * k)) == sum(abs(x * y) for x, y in zip(F[a], F[b]))
    G0, A0, k0 = cases.exact_gram(np.zeros((2, 3)))
    assert not G0.any() and not A0.any()


@pytest.mark.parametrize("n_dims", cases.GRAM_DIMS)
def test_the_bounds_hold_for_the_chain_and_tell_a_wrong_value(n_dims):
    """The derivation: the chain restated in NumPy (two roundings per step, so 2 M + 3 and 2 M + 6 roundings) stays within the
    bounds; a value moved by twice its bound, a float32 product and a matrix of another gamma do not."""
    X, tasks = cases.gram_inputs(n_dims)
    M = cases.chain_steps(n_dims)
    for rows, mean, scale, gamma in tasks[:4]:          # 1, 2, 17 and 33 rows
        Z = (X[rows] - mean) / scale
        K = cases.chain_gram(Z, "linear", gamma)
        n_bad, err, A = cases.linear_violations(K, Z, 2 * M + 3)
        assert n_bad == 0 and np.array_equal(K, K.T)
        if len(rows) >= 17:
            moved = K + 2 * (M + 3) * cases.U * np.abs(Z) @ np.abs(Z).T * (1 + 1e-3)
            assert cases.linear_violations(moved, Z)[0] == K.size
            low = (Z.astype(np.float32) @ Z.astype(np.float32).T).astype(np.float64)
            assert cases.linear_violations(low, Z)[0] > K.size // 2
        R = cases.chain_gram(Z, "rbf", gamma)
        assert cases.rbf_violations(R, Z, gamma, 2 * M + 6) == 0 and np.all(np.diagonal(R) == 1.0)
        if len(rows) >= 17:
            ref, x, _, _ = cases.rbf_reference(Z, gamma)
            assert cases.rbf_violations(R + 2 * cases.rbf_bound(x, ref, n_dims) * (1 + 1e-3), Z, gamma) == R.size
            assert cases.rbf_violations(cases.chain_gram(Z, "rbf", gamma * (1 + 1e-9)), Z, gamma) > R.size // 2


@pytest.mark.parametrize("kernel,C", cases.FINAL_FITS)
def test_the_goldens_rule_holds_for_the_restatement_of_the_final_fit(kernel, C):
    """The rule the device is held to in tests/test_svr_cache_gpu.py, on the restatement first: within max(4 x distance, 1e-9) of
    live scikit-learn -- and the distance itself within what the stopping tolerance 1e-3 allows (4 x 4e-3 on values of about 2,
    as tests/test_svr_fit_cpu.py derives it)."""
    pytest.importorskip("sklearn")
    Z, y, sk, sk_pred, ref_pred, tol = cases.final_fit_case(kernel, C)
    scale = np.max(np.abs(sk_pred))
    distance = np.max(np.abs(ref_pred - sk_pred)) / scale
    print("%s C=%g: distance %.3g, tol %.3g" % (kernel, C, distance, tol))
    assert tol >= 1e-9 and tol == max(4 * distance, 1e-9) and distance <= tol
    assert np.max(np.abs(ref_pred - sk_pred)) <= 4 * 4e-3
    assert np.all(np.abs(sk.dual_coef_) <= C) and np.all(np.diff(sk.support_) > 0)     # what to_sklearn_svr must look like
