"""GPU checks of the batched epsilon-SVR solver (svr_smo_kernel through paa_svr_tasks_f64 / audioTrainTest.svr_solve) and of the
SVR split sweep built on it (paa_svr_fit_splits_f64 / svr_split_fit_predict, evaluate_regression(svm_fit="device")).  The solver
checks are recomputed in NumPy from the returned state alone (beta, rho, the training predictions), so they do not depend on the
path the solver took; predictions are held against scikit-learn's through the goldens of scripts/make_svr_fit_golden.py (no
scikit-learn needed here)."""
import contextlib
import functools
import io
import warnings

import numpy as np
import pytest

import smo_ref
import svr_fit_ref
import train_ref
from pyaudioanalysis_amd import audioTrainTest
from test_svr_fit_cpu import KERNEL_NAMES, sweep_jobs

pytestmark = pytest.mark.gpu

EPS = 1e-3
EPSILON = 0.1
DIMS = (1, 8, 9, 136, 256)
CS = (0.001, 1.0, 10.0)
ROWS = (1, 2, 3, 31, 32, 33, 255, 256, 257, 1025)
N_SAMPLES = 1200


def fast_gram(Z, kernel, gamma, W=None):
    """The Gram matrix of the checks (the RBF distances in the expanded form: its cancellation error, about 1e-13 here, is far
    below the 1e-9 the checks ask for)."""
    W = Z if W is None else W
    if kernel == "linear":
        return Z @ W.T
    sz, sw = np.einsum("sd,sd->s", Z, Z), np.einsum("sd,sd->s", W, W)
    return np.exp(-gamma * np.maximum(sz[:, None] + sw[None, :] - 2.0 * (Z @ W.T), 0.0))


@functools.lru_cache(maxsize=None)
def batch(n_dims):
    """(X, y, tasks, names) of the solver batch at n_dims: every row count x C, then the special tasks.  The target is a linear
    function of two directions plus noise within 0.6 epsilon, so that a tube around the true function holds every row and the
    large tasks stop within some ten thousand iterations at C = 10 (with rows outside the tube, held at C, the linear kernel goes
    past 100 000); the task "mixed" has such rows.  A task standardises with the mean / deviation of its own rows."""
    rng = np.random.default_rng(200 + n_dims)
    U = rng.standard_normal((N_SAMPLES, n_dims))
    w = rng.standard_normal((2, n_dims)) / np.sqrt(n_dims)
    y = 2.0 + 0.3 * (U @ w[0]) + 0.5 * (U @ w[1]) + rng.uniform(-0.06, 0.06, N_SAMPLES)
    X = U * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    # the samples the special tasks own
    y[0:20] = 2.0 + rng.uniform(-0.09, 0.09, 20)        # in_tube: every target within epsilon of 2
    X[21] = X[20]                                       # identical: one point, two targets
    y[20], y[21] = 1.0, 3.0
    y[40:80] = np.where(np.arange(40) % 2 == 0, 5.0, -5.0) + rng.uniform(-0.5, 0.5, 40)         # all_at_C
    y[80:100] += np.where(np.arange(20) % 2 == 0, 1.0, -1.0) * rng.uniform(0.3, 0.6, 20)        # mixed: rows no tube can hold
    tasks, names = [], []

    def add(rows, C, name, stats=True, shrink=1.0):
        rows = np.asarray(rows)
        mean, scale = (X[rows].mean(axis=0), X[rows].std(axis=0) * shrink) if stats else (np.zeros(n_dims), np.ones(n_dims))
        scale = np.where(scale > 0, scale, 1.0)
        tasks.append((rows, mean, scale, C, None, EPSILON))
        names.append(name)

    for n in ROWS:
        for C in CS:
            add(100 + rng.permutation(N_SAMPLES - 100)[:n], C, "n%d_C%g" % (n, C), stats=n > 3)
    add(np.arange(20), 1.0, "in_tube")                  # the gap is the targets' range - 2 epsilon < 0: no iteration, beta = 0
    add([20, 21], 1.0, "identical", stats=False)        # eta = 0 between the variables of the two rows: the 1e-12 path
    # 20 targets near +5, 20 near -5, rows scaled to |z|^2 of about 1: 0.001 * 40 kernel values cannot bring a prediction within
    # epsilon of its target, so every beta ends at +-C, there is no free variable and rho is the midpoint
    add(np.arange(40, 80), 0.001, "all_at_C", shrink=np.sqrt(n_dims))
    add(np.concatenate([np.arange(80, 100), 100 + rng.permutation(N_SAMPLES - 100)[:44]]), 0.05, "mixed")
    return X, y, tasks, names


@functools.lru_cache(maxsize=None)
def solved(n_dims, kernel, iters_per_launch=0):
    X, y, tasks, names = batch(n_dims)
    return audioTrainTest.svr_solve(X, y, tasks, kernel=kernel, eps=EPS, iters_per_launch=iters_per_launch)


def dual_state(beta, K, targets, C):
    """(alpha [2 n], G [2 n]) of the returned beta: alpha_t = max(beta_t, 0), alpha_{t+n} = max(-beta_t, 0) -- for epsilon > 0
    libsvm never holds both variables of a row above zero at a stop that the checks accept -- and the gradient recomputed from
    it.  For epsilon > 0 ONLY: at epsilon = 0 the two variables of a row tie exactly, most states hold both above zero
    (tests/test_svr_edges_ref_cpu.py) and this helper must not be used."""
    alpha = np.concatenate([np.maximum(beta, 0.0), np.maximum(-beta, 0.0)])
    return alpha, svr_fit_ref.gradient(K, targets, alpha, EPSILON)


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
@pytest.mark.parametrize("n_dims", DIMS)
def test_solutions_meet_the_kkt_conditions(gpu_lib, n_dims, kernel):
    X, y, tasks, names = batch(n_dims)
    res = solved(n_dims, kernel)
    print("%s %d dims: iterations max %d median %d, launches %d" % (kernel, n_dims, res.iterations.max(), np.median(res.iterations),
                                                                   res.n_launches))
    assert np.all(res.status == audioTrainTest.SMO_CONVERGED)
    for t, (rows, mean, scale, C, _, _) in enumerate(tasks):
        beta, n = res.beta[t], len(rows)
        it = int(res.iterations[t])
        assert np.all(beta >= -C) and np.all(beta <= C), names[t]
        assert abs(np.sum(beta)) <= 4 * max(it, 1) * C * 2.0**-52, names[t]
        assert res.n_sv[t] == np.count_nonzero(beta), names[t]
        K = fast_gram((X[rows] - mean) / scale, kernel, 1.0 / n_dims)
        alpha, G = dual_state(beta, K, y[rows], C)
        s = svr_fit_ref.dual_signs(n)
        gmax, gmax2 = smo_ref.gap_and_sets(alpha, G, s, C)[:2]
        g_scale = max(1.0, np.max(np.abs(G)))
        assert gmax + gmax2 <= EPS * (1 + 1e-6) + 1e-9 * g_scale, (names[t], gmax + gmax2)
        assert abs(res.gap[t] - (gmax + gmax2)) <= 1e-9 * g_scale, names[t]
        rho = smo_ref.rho_of(alpha, G, s, C)
        assert abs(res.rho[t] - rho) <= 1e-9 * max(1.0, abs(rho)), (names[t], res.rho[t], rho)
        pred = K @ beta - res.rho[t]
        assert np.max(np.abs(res.train_pred[t] - pred)) <= 1e-9 * max(1.0, np.max(np.abs(pred))), names[t]
    t = names.index("in_tube")
    assert res.iterations[t] == 0 and not np.any(res.beta[t]) and res.n_sv[t] == 0
    lo, hi = y[:20].min(), y[:20].max()
    assert abs(res.rho[t] + (lo + hi) / 2) <= 1e-12 and np.all(np.abs(res.train_pred[t] - y[:20]) <= EPSILON)
    t = names.index("identical")
    assert res.iterations[t] >= 1 and np.array_equal(res.beta[t], [-1.0, 1.0])        # targets 1 and 3: both pushed to the bound
    t = names.index("all_at_C")
    assert np.array_equal(res.beta[t], np.where(y[40:80] > 0, 0.001, -0.001))
    if n_dims <= 9:                                     # variables at C and free ones in one task (64 rows at 136 dims interpolate)
        b = res.beta[names.index("mixed")]
        assert np.count_nonzero(np.abs(b) == 0.05) >= 10 and np.count_nonzero((b != 0) & (np.abs(b) < 0.05)) >= 2
    for n in (1, 2, 3):
        assert len(res.beta[names.index("n%d_C1" % n)]) == n


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_results_do_not_depend_on_the_launch_budget(gpu_lib, kernel):
    X, y, tasks, names = batch(8)
    keep = [t for t, task in enumerate(tasks) if len(task[0]) <= 33 or names[t] in ("n255_C1", "in_tube", "identical", "all_at_C", "mixed")]
    want = audioTrainTest.svr_solve(X, y, [tasks[t] for t in keep], kernel=kernel, eps=EPS)
    assert want.iterations.max() <= 20000, "a budget of one iteration per launch would take long"
    for ipl in (1, 7):
        got = audioTrainTest.svr_solve(X, y, [tasks[t] for t in keep], kernel=kernel, eps=EPS, iters_per_launch=ipl)
        assert got.n_launches > want.n_launches
        assert np.array_equal(got.iterations, want.iterations) and np.array_equal(got.status, want.status)
        assert np.array_equal(got.n_sv, want.n_sv)
        assert got.rho.tobytes() == want.rho.tobytes() and got.gap.tobytes() == want.gap.tobytes()
        for a, b in zip(got.beta + got.train_pred, want.beta + want.train_pred):
            assert a.tobytes() == b.tobytes()
    whole = solved(8, kernel)
    for k, t in enumerate(keep):
        assert whole.beta[t].tobytes() == want.beta[k].tobytes() and whole.train_pred[t].tobytes() == want.train_pred[k].tobytes()


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_a_task_does_not_depend_on_its_batch(gpu_lib, kernel):
    X, y, tasks, names = batch(9)
    t = names.index("n257_C1")
    alone = audioTrainTest.svr_solve(X, y, [tasks[t]], kernel=kernel, eps=EPS)
    others = [task for k, task in enumerate(tasks) if k != t and len(task[0]) <= 257]
    for pos in (0, len(others) // 2, len(others)):
        res = audioTrainTest.svr_solve(X, y, others[:pos] + [tasks[t]] + others[pos:], kernel=kernel, eps=EPS)
        assert res.beta[pos].tobytes() == alone.beta[0].tobytes() and res.train_pred[pos].tobytes() == alone.train_pred[0].tobytes()
        assert res.rho[pos].tobytes() == alone.rho[0].tobytes() and res.iterations[pos] == alone.iterations[0]
    whole = solved(9, kernel)
    assert whole.beta[t].tobytes() == alone.beta[0].tobytes()


def test_max_iter_is_reported_not_raised(gpu_lib):
    X, y, tasks, names = batch(8)
    t = names.index("n256_C10")
    assert solved(8, "linear").iterations[t] > 5
    with pytest.warns(Warning, match="max_iter=5"):
        res = audioTrainTest.svr_solve(X, y, [tasks[t], tasks[names.index("in_tube")]], kernel="linear", eps=EPS, max_iter=5)
    assert res.status.tolist() == [audioTrainTest.SMO_NOT_CONVERGED, audioTrainTest.SMO_CONVERGED] and res.iterations[0] == 5
    assert np.all(np.isfinite(res.beta[0])) and np.all(np.isfinite(res.train_pred[0]))
    assert np.isfinite(res.rho[0]) and np.isfinite(res.gap[0]) and res.gap[0] >= EPS
    assert np.all(np.abs(res.beta[0]) <= 10.0) and 2 <= np.count_nonzero(res.beta[0]) <= 10 and res.n_sv[0] == np.count_nonzero(res.beta[0])


def test_the_row_and_dims_limits_run(gpu_lib):
    """A task of 8192 rows at 256 dims (the largest LDS request) for three iterations."""
    rng = np.random.default_rng(9)
    n, d = audioTrainTest.smo_geometry()[2], audioTrainTest.smo_geometry()[5]
    X = rng.standard_normal((n, d))
    y = X[:, 0] + 0.1 * rng.standard_normal(n)
    task = (np.arange(n), np.zeros(d), np.ones(d), 1.0, None, EPSILON)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = audioTrainTest.svr_solve(X, y, [task], kernel="rbf", eps=EPS, max_iter=3)
    assert res.status[0] == audioTrainTest.SMO_NOT_CONVERGED and res.iterations[0] == 3
    beta = res.beta[0]
    assert np.all(np.abs(beta) <= 1.0) and 2 <= np.count_nonzero(beta) <= 6 and abs(np.sum(beta)) <= 1e-14
    sv = beta != 0
    pred = fast_gram(X, "rbf", 1.0 / d, X[sv]) @ beta[sv] - res.rho[0]
    assert np.max(np.abs(res.train_pred[0] - pred)) <= 1e-9 * max(1.0, np.max(np.abs(pred)))
    with pytest.raises(NotImplementedError, match="8192"):
        audioTrainTest.svr_solve(np.vstack([X, X[:1]]), np.append(y, 0.0), [(np.arange(n + 1),) + task[1:]])


@pytest.mark.parametrize("name", ["svr_fit_linear", "svr_fit_rbf"])
def test_sweep_against_scikit_learns_golden(gpu_lib, name):
    """Predictions within tol_pred of scikit-learn's; the golden's test lists are 0, 1, 31, 32, 33 and 97 rows long.  The training
    predictions, read from the solver's gradient, against the same job's rows scored as test rows."""
    g = train_ref.load_golden(name)
    jobs = sweep_jobs(g)
    kernel = KERNEL_NAMES[int(g["kernel_type"])]
    assert np.diff(g["test_off"]).tolist() == [0, 1, 31, 32, 33, 97]
    res = audioTrainTest.svr_split_fit_predict(g["X"], g["y"], jobs, kernel=kernel, epsilon=float(g["epsilon"]), eps=float(g["eps"]),
                                               train_pred=True)
    assert np.array_equal(res.test_off, g["test_off"]) and np.array_equal(res.train_off, g["train_off"])
    assert res.pred.shape == (int(g["test_off"][-1]),) and res.train_pred.shape == (int(g["train_off"][-1]),)
    assert np.all(res.status == audioTrainTest.SMO_CONVERGED) and np.all(res.iterations > 0) and res.n_launches >= 1
    for j, job in enumerate(jobs):
        a, b = int(g["test_off"][j]), int(g["test_off"][j + 1])
        pred, train_pred, its, status, n_sv = res.job(j)
        assert pred.shape == (b - a,) and train_pred.shape == (len(job[0]),)
        Z = (g["X"][job[0]] - job[2]) / job[3]
        if kernel == "rbf":
            assert res.gamma[j] == svr_fit_ref.scale_gamma(Z)
        if a == b:
            continue
        sk = g["sk_pred"][a:b]
        dist = np.max(np.abs(pred - sk)) / np.max(np.abs(sk))
        print("%s job %d: distance %.3g, tol_pred %.3g, n_sv %d (scikit-learn %d), iterations %d" % (name, j, dist, g["tol_pred"][j], n_sv,
                                                                                                      g["sk_n_sv"][j], its))
        assert dist <= g["tol_pred"][j], (name, j)
    # every job's training rows as its test rows: the scoring kernel against the gradient
    again = audioTrainTest.svr_split_fit_predict(g["X"], g["y"], [(job[0], job[0]) + job[2:] for job in jobs], kernel=kernel,
                                                 epsilon=float(g["epsilon"]), eps=float(g["eps"]))
    assert again.train_pred is None and np.array_equal(again.iterations, res.iterations) and np.array_equal(again.n_sv, res.n_sv)
    assert np.max(np.abs(again.pred - res.train_pred)) <= 1e-9 * max(1.0, np.max(np.abs(res.train_pred)))


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_test_list_lengths(gpu_lib, kernel):
    """Test lists of 0, 1, 31, 32, 33 and 97 rows (the scoring kernel serves 32 rows per workgroup) after one training list each:
    the predictions against beta and rho of the solver alone on the same rows, summed on the host."""
    X, y, tasks, names = batch(9)
    rows, mean, scale, C, _, _ = tasks[names.index("n33_C1")]
    rng = np.random.default_rng(7)
    tests = [rng.permutation(N_SAMPLES)[:n] for n in (0, 1, 31, 32, 33, 97)]
    gamma = 0.07
    sweep = audioTrainTest.svr_split_fit_predict(X, y, [(rows, te, mean, scale, C) for te in tests], kernel=kernel, gamma=gamma,
                                                 epsilon=EPSILON, eps=EPS)
    alone = audioTrainTest.svr_solve(X, y, [(rows, mean, scale, C, gamma, EPSILON)], kernel=kernel, eps=EPS)
    assert sweep.test_off.tolist() == [0, 0, 1, 32, 64, 97, 194] and np.all(sweep.iterations == alone.iterations[0])
    Z = (X[rows] - mean) / scale
    for j, te in enumerate(tests):
        pred = sweep.job(j)[0]
        want = smo_ref.gram((X[te] - mean) / scale, kernel, gamma, Z) @ alone.beta[0] - alone.rho[0]
        assert pred.shape == want.shape and np.all(np.abs(pred - want) <= 1e-9 * max(1.0, np.max(np.abs(want), initial=0.0)))


def _run(fn, *args, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = fn(*args, **kw)
    return ret, out.getvalue()


def regression_task(n=70, n_dims=6, seed=61):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, n_dims))
    y = 1.0 + np.tanh(U[:, 0]) + 0.5 * U[:, 1] + 0.1 * rng.standard_normal(n)
    return U * rng.uniform(0.5, 3.0, n_dims) + rng.uniform(-2.0, 2.0, n_dims), y


@pytest.mark.parametrize("kind", ["svm", "svm_rbf"])
def test_evaluate_regression_device_mode_equals_the_restatement(gpu_lib, kind):
    """Same seed, same splits: the chosen parameter is the restatement's, the errors agree to 1e-9 relative.  That asks for the
    same path through the solver, iteration by iteration.  The RBF kernel takes it at any C.  The linear dual is flat: from
    some hundred iterations on a rounding in the last place decides whether a variable returns to its bound exactly, the paths
    part, and two stops within the tolerance agree to about 1e-4 only (the linear goldens; a restatement whose kernel values are
    perturbed by one part in 1e16 parts from itself the same way at C = 0.05 on this data, and keeps its path up to C = 0.02).
    So the linear case tunes over values of C up to 0.02."""
    pytest.importorskip("sklearn")
    X, y = regression_task()
    params, n_exp = ([0.001, 0.05, 1.0] if kind == "svm_rbf" else [0.001, 0.005, 0.02]), 3
    np.random.seed(12)
    want_best, want_err, want_base, errs, train_errs = svr_fit_ref.evaluate_regression_ref(X, y, n_exp, kind, params)
    np.random.seed(12)
    (best, err, base), text = _run(audioTrainTest.evaluate_regression, X, y, n_exp, kind, params, svm_fit="device")
    print("%s: chosen %g (restatement %g), error %.17g (restatement %.17g), relative distance %.3g" % (kind, best, want_best, err, want_err,
                                                                                                     abs(err - want_err) / want_err))
    assert best == want_best and np.sort(errs)[1] - np.min(errs) > 1e-6 * np.min(errs)      # no tie for the restatement to lose
    assert abs(err - want_err) <= 1e-9 * want_err and abs(base - want_base) <= 1e-9 * want_base
    lines = text.splitlines()
    assert lines[0].split() == ["Param", "MSE", "T-MSE", "R-MSE"] and len(lines) == 1 + len(params)
    for line, param, e, te in zip(lines[1:], params, errs, train_errs):
        assert line.split()[:3] == ["%.4f" % param, "%.2f" % e, "%.2f" % te]
    assert sum(line.rstrip().endswith("best") for line in lines) == 1


def test_evaluate_regression_default_mode_is_the_parents(gpu_lib):
    """svm_fit="sklearn" (and no keyword at all): scikit-learn's fits and predictions in the parent's loop under the same seed."""
    sklearn_svm = pytest.importorskip("sklearn.svm")
    X, y = regression_task()
    params, n_exp = [0.05, 1.0], 2

    def fit(Z, labels, train, test, param):
        model = sklearn_svm.SVR(C=param, kernel="rbf").fit(Z[train], labels[train])
        return model.predict(Z[test]), model.predict(Z[train])

    np.random.seed(13)
    want = svr_fit_ref.evaluate_regression_ref(X, y, n_exp, "svm_rbf", params, fit)
    for kw in (dict(svm_fit="sklearn"), dict()):
        np.random.seed(13)
        (best, err, base), text = _run(audioTrainTest.evaluate_regression, X, y, n_exp, "svm_rbf", params, **kw)
        assert best == want[0] and abs(err - want[1]) <= 1e-9 * want[1] and abs(base - want[2]) <= 1e-9 * want[2]
        assert "best" in text
    for bad in (dict(svm_fit="gpu"),):
        with pytest.raises(ValueError):
            audioTrainTest.evaluate_regression(X, y, n_exp, "svm", params, **bad)
