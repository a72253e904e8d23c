"""GPU checks of the batched SMO solver (smo_kernel through paa_smo_tasks_f64 / audioTrainTest.smo_solve) and of the SVM split
sweep built on it (paa_svc_fit_splits_f64 / svm_split_fit_predict, evaluate_classifier(svm_fit="device")).  The solver checks
are recomputed in NumPy from the returned alpha alone, so they do not depend on the path the solver took; decision values and
labels are held against scikit-learn's through the goldens of scripts/make_smo_golden.py (no scikit-learn needed here)."""
import contextlib
import functools
import io
import warnings

import numpy as np
import pytest

import smo_ref
import train_ref
from pyaudioanalysis_amd import audioTrainTest
from test_smo_cpu import KERNEL_NAMES, binary_cases, near_rows, sweep_jobs

pytestmark = pytest.mark.gpu

EPS = 1e-3
DIMS = (1, 7, 8, 9, 136, 256)
CS = (0.001, 1.0, 20.0)
N_SAMPLES = 1200


def fast_gram(Z, kernel, gamma):
    """The Gram matrix of the checks (the RBF distances in the expanded form: its cancellation error, about 1e-13 here, is far
    below the 1e-9 the checks ask for)."""
    if kernel == "linear":
        return Z @ Z.T
    sq = np.einsum("sd,sd->s", Z, Z)
    return np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (Z @ Z.T), 0.0))


@functools.lru_cache(maxsize=None)
def batch(n_dims):
    """(X, tasks, names) of the solver batch at n_dims: every row count x C, then the special tasks.  Two overlapping Gaussian
    classes; a task standardises with the mean / deviation of its own rows."""
    T = audioTrainTest.smo_geometry()[0]
    rng = np.random.default_rng(100 + n_dims)
    y_all = np.where(np.arange(N_SAMPLES) % 2 == 0, 1.0, -1.0)
    X = rng.standard_normal((N_SAMPLES, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    X += 5.0 * y_all[:, None] / np.sqrt(n_dims)
    tasks, names = [], []

    def add(rows, signs, C, name, stats=True, shrink=1.0):
        rows = np.asarray(rows)
        mean, scale = (X[rows].mean(axis=0), X[rows].std(axis=0) * shrink) if stats else (np.zeros(n_dims), np.ones(n_dims))
        scale = np.where(scale > 0, scale, 1.0)
        tasks.append((rows, np.asarray(signs, dtype=np.float64), mean, scale, C, None))
        names.append(name)

    for n in (2, 3, T - 1, T, T + 1, 4 * T + 1):
        for C in CS:
            rows = rng.permutation(N_SAMPLES)[:n]
            if n == 2:
                rows = np.array([0, 1])                 # one per class
            if n == 3:
                rows = np.array([2, 5, 7])
            add(rows, y_all[rows], C, "n%d_C%g" % (n, C), stats=n > 3)
    add([10, 10], [1, -1], 1.0, "identical", stats=False)          # eta = 0: the 1e-12 path, both alpha end at C
    add(np.concatenate([[0], 1 + 2 * np.arange(64)]), [1] + [-1] * 64, 1.0, "one_against_64")
    rows = np.arange(40)
    # balanced, rows scaled to |z|^2 of about 1: 0.001 * 40 kernel values cannot reach the margin, every alpha ends at C, there
    # is no free row and rho is the midpoint
    add(rows, y_all[rows], 0.001, "all_at_C", shrink=np.sqrt(n_dims))
    return X, tasks, names


@functools.lru_cache(maxsize=None)
def solved(n_dims, kernel, iters_per_launch=0):
    X, tasks, names = batch(n_dims)
    return audioTrainTest.smo_solve(X, tasks, kernel=kernel, eps=EPS, iters_per_launch=iters_per_launch)


def test_geometry(gpu_lib):
    assert audioTrainTest.smo_geometry() == (256, 32, 8192, 32, 1024, 256)


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
@pytest.mark.parametrize("n_dims", DIMS)
def test_solutions_meet_the_kkt_conditions(gpu_lib, n_dims, kernel):
    X, tasks, names = batch(n_dims)
    res = solved(n_dims, kernel)
    assert np.all(res.status == audioTrainTest.SMO_CONVERGED)
    for t, (rows, y, mean, scale, C, _) in enumerate(tasks):
        ay = res.alpha_y[t]
        alpha = ay * y
        it = int(res.iterations[t])
        assert np.all(alpha >= 0) and np.all(alpha <= C), names[t]
        assert abs(np.sum(ay)) <= 4 * max(it, 1) * C * 2.0**-52, names[t]
        K = fast_gram((X[rows] - mean) / scale, kernel, 1.0 / n_dims)
        G = smo_ref.gradient(K, y, alpha)
        gmax, gmax2 = smo_ref.gap_and_sets(alpha, G, y, C)[:2]
        assert gmax + gmax2 <= EPS * (1 + 1e-6) + 1e-9 * max(1.0, np.max(np.abs(G))), (names[t], gmax + gmax2)
        assert abs(res.gap[t] - (gmax + gmax2)) <= 1e-9 * max(1.0, np.max(np.abs(G))), names[t]
        rho = smo_ref.rho_of(alpha, G, y, C)
        assert abs(res.rho[t] - rho) <= 1e-9 * max(1.0, abs(rho)), (names[t], res.rho[t], rho)
    t = names.index("identical")
    assert np.array_equal(res.alpha_y[t], [1.0, -1.0]) and res.iterations[t] == 1
    t = names.index("all_at_C")
    assert np.array_equal(np.abs(res.alpha_y[t]), np.full(40, 0.001))
    t = names.index("one_against_64")
    assert res.alpha_y[t][0] > 0 and res.iterations[t] >= 1


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_results_do_not_depend_on_the_launch_budget(gpu_lib, kernel):
    want = solved(7, kernel)
    for ipl in (1, 7):
        got = solved(7, kernel, ipl)
        assert got.n_launches > want.n_launches
        assert np.array_equal(got.iterations, want.iterations) and np.array_equal(got.status, want.status)
        assert got.rho.tobytes() == want.rho.tobytes() and got.gap.tobytes() == want.gap.tobytes()
        for a, b in zip(got.alpha_y, want.alpha_y):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_a_task_does_not_depend_on_its_batch(gpu_lib, kernel):
    X, tasks, names = batch(9)
    t = names.index("n257_C1")
    alone = audioTrainTest.smo_solve(X, [tasks[t]], kernel=kernel, eps=EPS)
    others = tasks[:t] + tasks[t + 1:]
    for pos in (0, len(others) // 2, len(others)):
        res = audioTrainTest.smo_solve(X, others[:pos] + [tasks[t]] + others[pos:], kernel=kernel, eps=EPS)
        assert res.alpha_y[pos].tobytes() == alone.alpha_y[0].tobytes()
        assert res.rho[pos].tobytes() == alone.rho[0].tobytes() and res.iterations[pos] == alone.iterations[0]
    whole = solved(9, kernel)
    assert whole.alpha_y[t].tobytes() == alone.alpha_y[0].tobytes()


def test_max_iter_is_reported_not_raised(gpu_lib):
    X, tasks, names = batch(8)
    t = names.index("n256_C20")
    assert solved(8, "linear").iterations[t] > 5
    with pytest.warns(Warning, match="max_iter=5"):
        res = audioTrainTest.smo_solve(X, [tasks[t], tasks[names.index("n2_C1")]], kernel="linear", eps=EPS, max_iter=5)
    assert res.status.tolist() == [audioTrainTest.SMO_NOT_CONVERGED, audioTrainTest.SMO_CONVERGED] and res.iterations[0] == 5
    assert np.all(np.isfinite(res.alpha_y[0])) and np.isfinite(res.rho[0]) and np.isfinite(res.gap[0]) and res.gap[0] >= EPS
    alpha = np.abs(res.alpha_y[0])
    assert np.all(alpha <= 20.0) and np.count_nonzero(alpha) >= 2


def test_the_row_and_dims_limits_run(gpu_lib):
    """A task of 8192 rows at 256 dims (the largest LDS request) for three iterations."""
    rng = np.random.default_rng(9)
    n, d = audioTrainTest.smo_geometry()[2], audioTrainTest.smo_geometry()[5]
    X = rng.standard_normal((n, d))
    y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    X += 0.1 * y[:, None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = audioTrainTest.smo_solve(X, [(np.arange(n), y, np.zeros(d), np.ones(d), 1.0, None)], kernel="rbf", eps=EPS, max_iter=3)
    assert res.status[0] == audioTrainTest.SMO_NOT_CONVERGED and res.iterations[0] == 3
    alpha = res.alpha_y[0] * y
    assert np.all(alpha >= 0) and np.all(alpha <= 1.0) and 2 <= np.count_nonzero(alpha) <= 6 and abs(np.sum(res.alpha_y[0])) <= 1e-14
    with pytest.raises(NotImplementedError, match="8192"):
        audioTrainTest.smo_solve(np.vstack([X, X[:1]]), [(np.arange(n + 1), np.append(y, 1.0), np.zeros(d), np.ones(d), 1.0, None)])


def test_decision_values_against_scikit_learns_golden(gpu_lib):
    g = train_ref.load_golden("smo_binary")
    X, lab = g["X"], g["labels"]
    tr, te = g["train_idx"], g["test_idx"]
    rows = np.concatenate([tr[lab[tr] == 0], tr[lab[tr] == 1]])
    y = np.where(lab[rows] == 0, 1.0, -1.0)
    for p, kernel, job, eps in binary_cases(g):
        res = audioTrainTest.smo_solve(X, [(rows, y, job[2], job[3], job[4], None)], kernel=kernel, eps=eps)
        assert res.status[0] == audioTrainTest.SMO_CONVERGED
        Z, Zq = (X[rows] - job[2]) / job[3], (X[te] - job[2]) / job[3]
        sv = res.alpha_y[0] != 0
        dec = smo_ref.gram(Zq, kernel, 1.0 / X.shape[1], Z[sv]) @ res.alpha_y[0][sv] - res.rho[0]
        sk = g[p + "sk_dec"]
        dist = np.max(np.abs(dec - sk)) / np.max(np.abs(sk))
        print("%s %s C=%g eps=%g: distance %.3g, tol_dec %.3g, iterations %d" % (p, kernel, job[4], eps, dist, float(g[p + "tol_dec"]),
                                                                                  res.iterations[0]))
        assert dist <= float(g[p + "tol_dec"]), p


@pytest.mark.parametrize("name", ["smo_sweep_linear", "smo_sweep_rbf"])
def test_sweep_against_scikit_learns_golden(gpu_lib, name):
    g = train_ref.load_golden(name)
    jobs = sweep_jobs(g)
    kernel = KERNEL_NAMES[int(g["kernel_type"])]
    res = audioTrainTest.svm_split_fit_predict(g["X"], g["labels"], jobs, kernel=kernel, eps=float(g["eps"]), decision=True)
    assert np.array_equal(res.test_off, g["test_off"]) and np.array_equal(np.diff(res.task_off), g["n_pairs"])
    assert res.decision.shape == (int(g["test_off"][-1]), 3) and np.all(res.status == audioTrainTest.SMO_CONVERGED)
    assert np.all(res.iterations > 0) and np.all(res.n_sv >= 2) and res.n_launches >= 1
    for j in range(len(jobs)):
        a, b = int(g["test_off"][j]), int(g["test_off"][j + 1])
        labels, dec, its, status, n_sv = res.job(j)
        assert labels.shape == (b - a,) and dec.shape == (b - a, int(g["n_pairs"][j]))
        assert np.array_equal(res.classes[j], np.unique(g["labels"][jobs[j][0]]))
        if a == b:
            continue
        sk = g["sk_dec"][a:b, :dec.shape[1]]
        dist = np.max(np.abs(dec - sk)) / np.max(np.abs(sk))
        print("%s job %d: distance %.3g, tol_dec %.3g" % (name, j, dist, g["tol_dec"][j]))
        assert dist <= g["tol_dec"][j], (name, j)
        assert not np.any(res.decision[a:b, dec.shape[1]:])
        near = near_rows(sk, g["tol_dec"][j])
        assert np.count_nonzero(near) <= 0.02 * (b - a)
        assert np.array_equal(labels[~near], g["sk_pred"][a:b][~near]), (name, j)
    # without the optional decision values: the same labels
    plain = audioTrainTest.svm_split_fit_predict(g["X"], g["labels"], jobs, kernel=kernel, eps=float(g["eps"]))
    assert plain.decision is None and np.array_equal(plain.label, res.label) and np.array_equal(plain.iterations, res.iterations)


def _run(fn, *args, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = fn(*args, **kw)
    return ret, out.getvalue()


@pytest.mark.parametrize("kind", ["svm", "svm_rbf"])
def test_evaluate_classifier_device_mode_equals_the_restatement(gpu_lib, kind):
    """Same seed, same splits; predictions may differ from the restatement's only on rows with a decision value within the
    cap of zero (tol_dec: the largest of the sweep golden of this kernel, the same data family; the seed is one under which at
    most 2 % of every split's test rows are such rows); C = 1 beats C = 0.0001 by far."""
    pytest.importorskip("sklearn")
    feats = train_ref.class_features((100, 80, 60), 20, seed=31, spread=2.5)
    names, params, n_exp, pct = ["a", "b", "c"], [0.0001, 1.0], 3, 0.75
    tol = float(np.max(train_ref.load_golden("smo_sweep_rbf" if kind == "svm_rbf" else "smo_sweep_linear")["tol_dec"]))
    np.random.seed(10)
    want_best, want_cms, want_preds, splits, decs = smo_ref.evaluate_svm_sweep_ref(feats, names, kind, params, 0, n_exp, pct)
    acc = [np.trace(cm) / np.sum(cm) for cm in want_cms]
    assert want_best == 1.0 and acc[1] - acc[0] > 0.3           # a clear winner
    np.random.seed(10)
    (best, cms, preds), text = _run(audioTrainTest.evaluate_classifier_full, feats, names, kind, params, 0, None, n_exp=n_exp,
                                    train_percentage=pct, svm_fit="device")
    assert best == want_best and "best Acc" in text
    X, y = train_ref.features_to_matrix(feats)
    moved = 0
    for p in range(len(params)):
        for e in range(n_exp):
            near = near_rows(decs[p][e], tol)
            assert np.count_nonzero(near) <= 0.02 * len(near)
            got, want = np.array(preds[p][e], dtype=np.float64), np.array(want_preds[p][e], dtype=np.float64)
            assert got.shape == want.shape == (len(splits[p][e][1]),)
            assert np.array_equal(got[~near], want[~near]), (p, e)
            moved += int(np.count_nonzero(got != want))
    for cm, want_cm in zip(cms, want_cms):
        assert np.sum(np.abs(np.asarray(cm) - want_cm)) <= 2 * moved + 1e-6
    ret = _run(audioTrainTest.evaluate_classifier, feats, names, kind, params, 0, None, n_exp=n_exp, train_percentage=pct,
               svm_fit="device")[0]
    assert ret == want_best


def test_evaluate_classifier_default_mode_is_the_parents(gpu_lib):
    """svm_fit="sklearn" (and no keyword at all): the predictions of the scikit-learn restatement of tests/train_ref.py under
    the same seed, as before the device mode existed."""
    pytest.importorskip("sklearn")
    feats = train_ref.three_class_features()
    names, params, n_exp, pct = ["a", "b", "c"], [0.5, 5.0], 2, 0.8
    for kw in (dict(svm_fit="sklearn"), dict()):
        np.random.seed(3)
        want_ret, want_cms, want_preds, want_text = train_ref.evaluate(
            feats, names, params, 1, n_exp, train_ref.random_split_source(sum(len(f) for f in feats), pct), train_ref.sklearn_fit("svm"),
            train_ref.sklearn_classify)
        np.random.seed(3)
        (ret, cms, preds), text = _run(audioTrainTest.evaluate_classifier_full, feats, names, "svm", params, 1, None, n_exp=n_exp,
                                       train_percentage=pct, **kw)
        assert ret == want_ret and text == want_text
        assert np.array_equal(np.array(cms), want_cms)
        assert np.array_equal(np.concatenate([p for row in preds for p in row]), np.concatenate(want_preds))


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_solver_alone_against_the_sweep(gpu_lib, kernel):
    """Every pair task of a two-job sweep, solved by smo_solve on the rows the sweep builds for it (class a's rows in train-list
    order, then class b's, signs +1 / -1): the iterations and status the sweep reports, and the sweep's decision values against
    alpha_y / rho of the solver alone, recomputed on the host as test_decision_values_against_scikit_learns_golden does, within
    that golden case's tol_dec.  The smo_binary golden's matrix, splits and statistics under three classes (class 1 split in two)."""
    g = train_ref.load_golden("smo_binary")
    X, tr, te = g["X"], g["train_idx"], g["test_idx"]
    lab = np.where((g["labels"] == 1) & (np.arange(X.shape[0]) % 2 == 1), 2, g["labels"])
    cases = [(p, job) for p, name, job, eps in binary_cases(g) if name == kernel and eps == EPS and job[4] >= 1.0]
    assert len(cases) == 2
    sweep = audioTrainTest.svm_split_fit_predict(X, lab, [job for p, job in cases], kernel=kernel, eps=EPS, decision=True)
    assert [c.tolist() for c in sweep.classes] == [[0, 1, 2]] * 2 and sweep.task_off.tolist() == [0, 3, 6]
    for j, (p, job) in enumerate(cases):
        pairs = [(a, b) for a in range(3) for b in range(a + 1, 3)]
        tasks = [(np.concatenate([tr[lab[tr] == a], tr[lab[tr] == b]]),
                  np.concatenate([np.ones(np.count_nonzero(lab[tr] == a)), -np.ones(np.count_nonzero(lab[tr] == b))]),
                  job[2], job[3], job[4], None) for a, b in pairs]
        alone = audioTrainTest.smo_solve(X, tasks, kernel=kernel, eps=EPS)
        labels, dec, its, status, n_sv = sweep.job(j)
        assert np.array_equal(alone.iterations, its) and np.array_equal(alone.status, status)
        assert np.array_equal([np.count_nonzero(a) for a in alone.alpha_y], n_sv)
        Zq = (X[te] - job[2]) / job[3]
        for t, task in enumerate(tasks):
            sv = alone.alpha_y[t] != 0
            host = smo_ref.gram(Zq, kernel, 1.0 / X.shape[1], ((X[task[0]] - job[2]) / job[3])[sv]) @ alone.alpha_y[t][sv] - alone.rho[t]
            dist = np.max(np.abs(dec[:, t] - host)) / np.max(np.abs(host))
            print("%s job %d pair %s: distance %.3g, tol_dec %.3g, iterations %d" % (kernel, j, pairs[t], dist, float(g[p + "tol_dec"]), its[t]))
            assert dist <= float(g[p + "tol_dec"]), (p, t)
