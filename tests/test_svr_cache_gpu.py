"""GPU checks of the SVR solver's resident kernel matrix (DESIGN K22: svr_standardise_kernel, svr_gram_kernel,
svr_smo_cached_kernel through paa_svr_tasks_cached_f64 / paa_svr_fit_splits_cached_f64 / paa_svr_gram_f64) and of what is built
on it: svr_solve / svr_split_fit_predict / evaluate_regression(kernel_cache="gram"), train_svm_regression_device, to_sklearn_svr
and feature_extraction_train_regression(final_fit="device").  The gate of the cached solver is byte equality with the recomputing
one: no tolerance applies.  The inputs, the exact restatement and the bounds are tests/svr_cache_cases.py's."""
import contextlib
import functools
import io
import os
import pickle
import warnings

import numpy as np
import pytest

import svr_cache_cases as cases
from pyaudioanalysis_amd import audioTrainTest as aT
from test_svr_fit_gpu import DIMS, EPS, EPSILON, N_SAMPLES, batch, regression_task, solved

pytestmark = pytest.mark.gpu

T = aT.SVR_GRAM_TILE


@functools.lru_cache(maxsize=None)
def extra_tasks(n_dims):
    """Tasks of T - 1, T and T + 1 rows of the batch's samples, T the Gram kernel's tile edge, and of 2 T + 1 rows (three tiles a
    side, the last of one row)."""
    X, y, tasks, names = batch(n_dims)
    rng = np.random.default_rng(300 + n_dims)
    out = []
    for n in (T - 1, T, T + 1, 2 * T + 1):
        rows = 100 + rng.permutation(N_SAMPLES - 100)[:n]
        out.append((rows, X[rows].mean(axis=0), X[rows].std(axis=0), 1.0, None, EPSILON))
    return out


@functools.lru_cache(maxsize=None)
def uncached(n_dims, kernel):
    """The recomputing solver's results for batch(n_dims) + extra_tasks(n_dims), task by task: the batch's from the solve that
    tests/test_svr_fit_gpu.py shares, the extra tasks' from a call of their own (a task does not depend on its batch)."""
    X, y, tasks, names = batch(n_dims)
    a, b = solved(n_dims, kernel), aT.svr_solve(X, y, extra_tasks(n_dims), kernel=kernel, eps=EPS)
    assert not a.cached.any() and not b.cached.any()
    return [fields(r, t) for r in (a, b) for t in range(len(r.rho))]


def fields(res, t):
    """Every output of task t as bytes and integers."""
    return (res.beta[t].tobytes(), res.train_pred[t].tobytes(), res.rho[t].tobytes(), res.gap[t].tobytes(), int(res.iterations[t]),
            int(res.status[t]), int(res.n_sv[t]))


def all_tasks(n_dims):
    X, y, tasks, names = batch(n_dims)
    return X, y, list(tasks) + list(extra_tasks(n_dims)), list(names) + ["tile%+d" % d for d in (-1, 0, 1)] + ["three_tiles"]


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
@pytest.mark.parametrize("n_dims", DIMS)
def test_the_cached_solver_is_byte_equal_to_the_recomputing_one(gpu_lib, n_dims, kernel):
    X, y, tasks, names = all_tasks(n_dims)
    assert len(tasks) == 34 + 4
    want = uncached(n_dims, kernel)
    got = aT.svr_solve(X, y, tasks, kernel=kernel, eps=EPS, kernel_cache="gram")
    assert got.cached.dtype == bool and got.cached.all()
    for t, name in enumerate(names):
        assert fields(got, t) == want[t], (name, got.iterations[t], want[t][4])
    print("%s %d dims: iterations max %d" % (kernel, n_dims, got.iterations.max()))
    assert np.all(got.status == aT.SMO_CONVERGED) and got.iterations.max() > 0


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_cached_results_do_not_depend_on_the_launch_budget(gpu_lib, kernel):
    X, y, tasks, names = all_tasks(8)
    keep = [t for t, task in enumerate(tasks) if len(task[0]) <= 2 * T + 1 or names[t] in ("n255_C1", "in_tube", "identical", "all_at_C", "mixed")]
    want = uncached(8, kernel)
    assert max(want[t][4] for t in keep) <= 20000, "a budget of one iteration per launch would take long"
    launches = []
    for ipl in (1, 7, 0):
        got = aT.svr_solve(X, y, [tasks[t] for t in keep], kernel=kernel, eps=EPS, iters_per_launch=ipl, kernel_cache="gram")
        assert got.cached.all()
        for k, t in enumerate(keep):
            assert fields(got, k) == want[t], (ipl, names[t])
        launches.append(got.n_launches)
    assert launches[0] > launches[1] > launches[2]


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_a_cached_task_does_not_depend_on_its_batch(gpu_lib, kernel):
    X, y, tasks, names = all_tasks(9)
    t = names.index("n257_C1")
    want = uncached(9, kernel)[t]
    alone = aT.svr_solve(X, y, [tasks[t]], kernel=kernel, eps=EPS, kernel_cache="gram")
    assert alone.cached.all() and fields(alone, 0) == want
    others = [task for k, task in enumerate(tasks) if k != t and len(task[0]) <= 257]
    for pos in (0, len(others) // 2, len(others)):
        res = aT.svr_solve(X, y, others[:pos] + [tasks[t]] + others[pos:], kernel=kernel, eps=EPS, kernel_cache="gram")
        assert res.cached.all() and fields(res, pos) == want, pos


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_chunking_keeps_every_byte_and_reports_what_the_packing_rule_implies(gpu_lib, kernel):
    X, y, tasks, names = all_tasks(9)
    rows = [len(task[0]) for task in tasks]
    want = uncached(9, kernel)
    big = cases.matrix_bytes(1025)
    for budget, n_chunks in ((sum(cases.matrix_bytes(n) for n in rows), 1), (big, None), (big - 1, None), (8, None)):
        got = aT.svr_solve(X, y, tasks, kernel=kernel, eps=EPS, kernel_cache="gram", cache_bytes=budget)
        chunk_of = aT.svr_cache_chunks(rows, budget)
        assert np.array_equal(got.cached, chunk_of >= 0) and np.array_equal(got.cached, cases.expected_cached(rows, budget)), budget
        if n_chunks is not None:
            assert chunk_of.max() + 1 == n_chunks
        for t, name in enumerate(names):
            assert fields(got, t) == want[t], (budget, name)
        if budget == big:
            assert got.cached.all() and chunk_of.max() >= 3        # each 1025-row matrix fills a chunk alone
        if budget == big - 1:
            assert [names[t] for t in np.flatnonzero(~got.cached)] == ["n1025_C0.001", "n1025_C1", "n1025_C10"]
        if budget == 8:
            assert [rows[t] for t in np.flatnonzero(got.cached)] == [1, 1, 1]


def test_offsets_beyond_4_gib(gpu_lib):
    """Nine tasks of 8192 rows x 1 dim under a budget of 5 GiB: one chunk of 4.5 GiB, so the last task's matrix begins at byte
    offset 4 GiB; three iterations each."""
    rng = np.random.default_rng(77)
    n = cases.MAX_ROWS
    X = rng.standard_normal((n + 500, 1))
    y = np.tanh(X[:, 0]) + 0.2 * rng.standard_normal(n + 500)
    tasks = [(rng.permutation(n + 500)[:n], np.array([0.1 * k]), np.array([1.0 + 0.05 * k]), 0.5 + k, 0.3 + 0.1 * k, EPSILON) for k in range(9)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = aT.svr_solve(X, y, tasks, kernel="rbf", eps=EPS, max_iter=3)
        got = aT.svr_solve(X, y, tasks, kernel="rbf", eps=EPS, max_iter=3, kernel_cache="gram", cache_bytes=5 << 30)
    assert got.cached.all() and not want.cached.any() and aT.svr_cache_chunks([n] * 9, 5 << 30).tolist() == [0] * 9
    assert np.all(got.iterations == 3) and np.all(got.status == aT.SMO_NOT_CONVERGED)
    for t in range(9):
        assert fields(got, t) == fields(want, t), t
        assert 2 <= np.count_nonzero(got.beta[t]) <= 6


@pytest.mark.parametrize("n_dims", cases.GRAM_DIMS)
def test_the_gram_kernel_alone(gpu_lib, n_dims):
    X, tasks = cases.gram_inputs(n_dims)
    assert [len(task[0]) for task in tasks] == list(cases.GRAM_ROWS)
    lin, qd = aT.svr_kernel_matrix(X, tasks, "linear", with_qd=True)
    rbf, qd_rbf = aT.svr_kernel_matrix(X, tasks, "rbf", with_qd=True)
    for t, (rows, mean, scale, gamma) in enumerate(tasks):
        n = len(rows)
        Z = (X[rows] - mean) / scale
        assert lin[t].shape == (n, n) and rbf[t].shape == (n, n)
        assert lin[t].tobytes() == lin[t].T.copy().tobytes() and rbf[t].tobytes() == rbf[t].T.copy().tobytes()
        assert np.diagonal(lin[t]).tobytes() == qd[t].tobytes()               # the recomputing solver's own K_tt
        assert np.all(np.diagonal(rbf[t]) == 1.0) and np.all(qd_rbf[t] == 1.0)
        n_bad, err, A = cases.linear_violations(lin[t], Z)
        worst = max((float(e) / float(a) for e, a in zip(err.ravel(), A.ravel()) if a), default=0.0) / cases.U
        print("%d dims, %d rows: linear error at most %.3g u sum |z z'| (bound %d u)" % (n_dims, n, worst, cases.chain_steps(n_dims) + 3))
        assert n_bad == 0
        assert cases.rbf_violations(rbf[t], Z, gamma) == 0
    # alone or in another batch, in another place: the same bytes
    again = aT.svr_kernel_matrix(X, tasks[::-1], "rbf")
    for t in range(len(tasks)):
        assert again[len(tasks) - 1 - t].tobytes() == rbf[t].tobytes()


@pytest.mark.parametrize("kernel,C", cases.FINAL_FITS)
def test_the_final_fit_and_its_scikit_learn_model(gpu_lib, kernel, C, tmp_path):
    pytest.importorskip("sklearn")
    import sklearn.svm
    Z, y, sk, sk_pred, ref_pred, tol = cases.final_fit_case(kernel, C)
    model, train_error = aT.train_svm_regression_device(Z, y, C, kernel)
    assert model.fit_result.cached.all() and model.fit_result.status[0] == aT.SMO_CONVERGED
    other, other_error = aT.train_svm_regression_device(Z, y, C, kernel, kernel_cache="none")
    assert fields(other.fit_result, 0) == fields(model.fit_result, 0) and other_error == train_error
    svr = aT.to_sklearn_svr(model)
    assert type(svr) is sklearn.svm.SVR
    pred = svr.predict(Z)
    scale = np.max(np.abs(sk_pred))
    distance = np.max(np.abs(pred - sk_pred)) / scale
    print("%s C=%g: device distance %.3g, restatement %.3g, tol %.3g" % (kernel, C, distance, np.max(np.abs(ref_pred - sk_pred)) / scale, tol))
    assert distance <= tol
    assert np.all(np.diff(svr.support_) > 0) and svr.support_.dtype == np.int32
    assert np.all(np.abs(svr.dual_coef_) <= C) and svr.dual_coef_.shape == (1, len(svr.support_)) and np.all(svr.dual_coef_ != 0)
    assert np.array_equal(svr.support_vectors_, Z[svr.support_]) and svr.intercept_[0] == -model.fit_result.rho[0]
    assert svr.shape_fit_ == Z.shape and svr.n_features_in_ == 12 and svr.fit_status_ == 0
    assert svr._probA.size == 0 and svr._probB.size == 0
    if kernel == "rbf":
        assert svr._gamma == sk._gamma
    for name in ("support_", "support_vectors_", "dual_coef_", "intercept_", "_n_support", "shape_fit_", "_sparse"):
        a, b = getattr(svr, name), getattr(sk, name)    # the attributes have scikit-learn's own types and shapes
        assert type(a) is type(b) and (not isinstance(b, np.ndarray) or (a.dtype == b.dtype and a.ndim == b.ndim)), name
    assert svr.n_support_.tolist() == [len(svr.support_)]
    # the pickle round trip, in the reference's format
    path = str(tmp_path / "model")
    with open(path, "wb") as fo:
        pickle.dump(svr, fo)
    with open(path, "rb") as fo:
        back = pickle.load(fo)
    assert np.array_equal(back.predict(Z), pred)
    # the device's own predictions of the model, and the training error from the gradient
    dev = aT.regress([back], "svm_rbf" if kernel == "rbf" else "svm", np.ascontiguousarray(Z.T), np.zeros(12), np.ones(12))[0]
    assert np.max(np.abs(dev - pred)) <= 1e-9 * np.max(np.abs(pred))
    assert aT.regression_wrapper(back, "svm", Z[5]) == pytest.approx(pred[5], rel=1e-9)
    assert abs(train_error - np.mean(np.abs(pred - y))) <= 1e-9 * max(1.0, train_error)


def _run(fn, *args, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = fn(*args, **kw)
    return ret, out.getvalue()


@pytest.mark.parametrize("kind", ["svm", "svm_rbf"])
def test_evaluate_regression_with_the_cache_returns_exactly_what_it_returns_without(gpu_lib, kind):
    pytest.importorskip("sklearn")
    X, y = regression_task()
    params = [0.001, 0.05, 1.0] if kind == "svm_rbf" else [0.001, 0.005, 0.02]
    runs = []
    for kw in (dict(kernel_cache="none"), dict(kernel_cache="gram"), dict(kernel_cache="gram", cache_bytes=8 * 63 * 63), dict()):
        np.random.seed(12)
        runs.append(_run(aT.evaluate_regression, X, y, 3, kind, params, svm_fit="device", **kw))
    for ret, text in runs[1:]:
        assert ret == runs[0][0] and text == runs[0][1]
    assert "best" in runs[0][1]


def test_feature_extraction_train_regression_final_fit_device(gpu_lib, tmp_path):
    """A folder of short synthetic WAVs and one CSV: the model file is the device's fit, a pickled sklearn.svm.SVR that
    load_model(..., is_regression=True) and file_regression read unchanged."""
    pytest.importorskip("sklearn")
    import sklearn.svm
    from scipy.io import wavfile
    folder = str(tmp_path / "clips")
    os.makedirs(folder)
    rng = np.random.default_rng(31)
    fs, rows = 16000, []
    for k in range(12):
        f0 = 200.0 + 60.0 * k
        t = np.arange(int(1.5 * fs)) / fs
        x = 6000 * np.sin(2 * np.pi * f0 * t) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t)) + 300 * rng.standard_normal(t.size)
        wavfile.write(os.path.join(folder, "clip%02d.wav" % k), fs, x.astype(np.int16))
        rows.append("clip%02d.wav,%.3f" % (k, f0 / 100.0 + 0.1 * rng.standard_normal()))
    with open(os.path.join(folder, "pitch.csv"), "wt") as fo:
        fo.write("\n".join(rows) + "\n")
    model_name = str(tmp_path / "model")
    np.random.seed(3)
    (errors, base_errors, best), text = _run(aT.feature_extraction_train_regression, folder, 0.5, 0.5, 0.05, 0.05, "svm_rbf", model_name,
                                             svm_fit="device", final_fit="device", kernel_cache="gram")
    assert len(errors) == len(base_errors) == len(best) == 1 and "Selected params" in text
    assert os.path.isfile(model_name + "_pitch") and os.path.isfile(model_name + "_pitchMEANS")
    with open(model_name + "_pitch", "rb") as fo:
        raw = pickle.load(fo)
    assert type(raw) is sklearn.svm.SVR and raw.C == best[0] and raw.kernel == "rbf"
    assert np.all(np.diff(raw.support_) > 0) and np.all(np.abs(raw.dual_coef_) <= best[0])
    loaded = aT.load_model(model_name + "_pitch", True)
    model, mean, std = loaded[:3]
    assert type(model) is sklearn.svm.SVR and tuple(loaded[3:7]) == (0.5, 0.5, 0.05, 0.05)
    assert np.array_equal(model.dual_coef_, raw.dual_coef_) and len(mean) == len(std) == model.n_features_in_
    # the file is the device's fit at the chosen C: the same bytes as a fit of our own on the standardised features
    feats = aT.aF.multiple_directory_feature_extraction([folder], 0.5, 0.5, 0.05, 0.05, compute_beat=False)[0][0]
    names = sorted(os.listdir(folder))
    assert feats.shape[0] == 12 and names[0] == "clip00.wav"
    results, tasks = aT.file_regression(os.path.join(folder, "clip03.wav"), model_name, "svm_rbf")
    assert tasks == ["pitch"] and len(results) == 1 and np.isfinite(results[0])
    z = (feats - np.asarray(mean)) / np.asarray(std)
    by_model = model.predict(z)
    assert min(abs(results[0] - v) for v in by_model) <= 1e-9 * max(1.0, abs(results[0]))
