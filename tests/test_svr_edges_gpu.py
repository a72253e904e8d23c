"""GPU checks of the PATH the batched epsilon-SVR solver takes (svr_smo_kernel through audioTrainTest.svr_solve) and of its
per-task parameters at their edges.  tests/test_svr_fit_gpu.py pins where the solver ends (the KKT conditions within eps); a
solver that breaks one of libsvm's rules -- the tie-break of a selection, above all between the two variables of one row at
epsilon = 0, the second-order choice of j, a clip of the two-variable update, the TAU path, a task's own epsilon or gamma -- still
ends there.  Here the restatement of tests/svr_fit_ref.py is followed step by step on the inputs of tests/svr_edge_cases.py,
whose every selection is decided far above rounding, or tied exactly (tests/test_svr_edges_ref_cpu.py asserts that, and that each
such wrong solver is told apart by what is compared here), so a correct solver takes the same steps.

Observed on an MI355X (the figures the tests print): after 1 .. 8 steps and at the stop |beta - beta_ref| is at most 1.11e-15 C
under the linear kernel and 8.33e-16 C under the RBF kernel (bound 1e-9 C).  A first version of the set held a 70-row task that
the kernel finished in 70 iterations against the restatement's 69: a value met C by alpha_i - alpha_j = 0 in NumPy and stayed
one ulp inside it under the kernel's fused multiply-add (reproduced on the CPU with an exact fma in the restatement's gradient
update).  Both runs obey libsvm's rules; the inputs now keep such values away from the bounds (bound_margin, asserted in
tests/test_svr_edges_ref_cpu.py)."""
import functools
import warnings

import numpy as np
import pytest

import smo_ref
import svr_edge_cases as cases
import svr_fit_ref as ref
from pyaudioanalysis_amd import audioTrainTest

pytestmark = pytest.mark.gpu

STEPS = 8
BETA_TOL = 1e-9                 # of C: ALPHA_TOL of tests/test_smo_edges_gpu.py, the project's gate for sums of kernel values
VALUE_TOL = 1e-9                # of max(1, |value|): rho, the gap and the training predictions
observed = {"linear": 0.0, "rbf": 0.0}


def quiet_solve(*args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return audioTrainTest.svr_solve(*args, **kw)


def quiet_sweep(*args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return audioTrainTest.svr_split_fit_predict(*args, **kw)


def task_gram(X, n_dims, kernel, task):
    return smo_ref.gram(cases.standardised(X, task), kernel, 1.0 / n_dims if task[4] is None else task[4])


def same_bytes(a, b):
    return (a.iterations.tobytes() == b.iterations.tobytes() and a.status.tobytes() == b.status.tobytes()
            and a.rho.tobytes() == b.rho.tobytes() and a.gap.tobytes() == b.gap.tobytes() and a.n_sv.tobytes() == b.n_sv.tobytes()
            and all(x.tobytes() == y.tobytes() for x, y in zip(a.beta + a.train_pred, b.beta + b.train_pred)))


def close(got, want, scale=None):
    scale = max(1.0, float(np.max(np.abs(want)))) if scale is None else scale
    return bool(np.all(np.abs(got - want) <= VALUE_TOL * scale))


@pytest.mark.parametrize("key", list(cases.trajectory_batches()), ids=lambda k: "d%d_%s_eps%g" % k)
def test_the_solver_takes_the_restatements_steps(gpu_lib, key):
    """After each of the first 8 steps and at the stop: the restatement's iteration count and status, its beta within 1e-9 C and
    n_sv = the rows with beta != 0; after each of the first 8 steps its non-zero set too; at the stop its rho, gap and training
    predictions (G[:n] - epsilon + y - rho of the restatement's own gradient) within 1e-9 max(1, |.|).  The tasks of a key are one
    batch, among them the pairs that differ in epsilon alone and in gamma alone."""
    n_dims, kernel, eps = key
    batch = cases.trajectory_batches()[key]
    X, y = cases.trajectory_matrix(n_dims)
    grams = [task_gram(X, n_dims, kernel, t.task) for t in batch]
    worst = 0.0
    for m in list(range(1, STEPS + 1)) + [10**7]:
        res = quiet_solve(X, y, [t.task for t in batch], kernel=kernel, eps=eps, max_iter=m)
        for pos, (t, K) in enumerate(zip(batch, grams)):
            rows, mean, scale, C, gamma, epsilon = t.task
            n = len(rows)
            alpha, G, rho, it, gap, status = ref.solve(K, y[rows], C, epsilon, eps, max_iter=m)
            beta = alpha[:n] - alpha[n:]
            assert (int(res.iterations[pos]), int(res.status[pos])) == (it, status), (t.name, m)
            if m <= STEPS:
                assert np.array_equal(np.flatnonzero(res.beta[pos]), np.flatnonzero(beta)), (t.name, m)
            dist = float(np.max(np.abs(res.beta[pos] - beta))) / C
            worst = max(worst, dist)
            assert dist <= BETA_TOL, (t.name, m, dist)
            assert res.n_sv[pos] == np.count_nonzero(res.beta[pos]), (t.name, m)
            if status == ref.STATUS_CONVERGED:
                assert close(res.rho[pos], rho) and close(res.gap[pos], gap, max(1.0, float(np.max(np.abs(G))))), (t.name, m, res.rho[pos], rho)
                assert close(res.train_pred[pos], G[:n] - epsilon + y[rows] - rho), (t.name, m)
    observed[kernel] = max(observed[kernel], worst)
    print("%s: largest |beta - beta_ref| / C over %d steps and at the stop %.3g (so far, %s: %.3g)" % ("d%d_%s_eps%g" % key, STEPS, worst,
                                                                                                    kernel, observed[kernel]))


def test_exact_ties_go_to_the_greatest_index(gpu_lib):
    """One step on every tie layout, all in one batch: exactly the rows of the restatement's (i, j) are touched -- the greatest
    index among the rows of the greatest target, n + the greatest index among the tied best rows of the least -- and beta is
    the restatement's, bit for bit (integer samples and targets: everything at step 1 is exact up to the one division)."""
    X, y = cases.tie_matrix()
    layouts = cases.tie_layouts()
    res = quiet_solve(X, y, [lay.task for lay in layouts], kernel="linear", max_iter=1)
    bad = []
    for pos, lay in enumerate(layouts):
        rows, mean, scale, C, _, epsilon = lay.task
        n = len(rows)
        alpha = ref.solve(smo_ref.gram(cases.standardised(X, lay.task), "linear", 0), y[rows], C, epsilon, max_iter=1)[0]
        assert np.array_equal(np.flatnonzero(alpha), [lay.i, lay.j])
        beta, got = alpha[:n] - alpha[n:], res.beta[pos]
        if not (np.array_equal(np.flatnonzero(got), sorted((lay.i, lay.j - n))) and np.all(got == beta) and res.iterations[pos] == 1
                and res.n_sv[pos] == 2):
            bad.append((lay.name, np.flatnonzero(got).tolist()))
    assert not bad, bad


DEGENERATE_KEYS = [key for key, batch in cases.trajectory_batches().items() if key[0] <= 9 and len(batch) >= 2]


@pytest.mark.parametrize("key", DEGENERATE_KEYS, ids=lambda k: "d%d_%s_eps%g" % k)
def test_degenerate_tasks_stop_at_once_and_disturb_nobody(gpu_lib, key):
    """One row, rows of one target, targets within the tube, under epsilon 0 and 0.1: converged in 0 iterations with beta = 0,
    n_sv = 0, the restatement's gap (y_max - y_min - 2 epsilon, exactly 0 for equal targets at epsilon 0) and rho EQUAL to
    smo_ref.rho_of's: the midpoint of a minimum and a maximum does not depend on the order they are found in.  all_at_C: every
    beta at +-C exactly, rho the midpoint over the gradient of that beta.  The ordinary tasks around them are bit-identical to
    the same tasks solved without them."""
    n_dims, kernel, eps = key
    assert {k[:2] for k in DEGENERATE_KEYS} == {(1, "linear"), (1, "rbf"), (9, "linear"), (9, "rbf")}
    X, y = cases.trajectory_matrix(n_dims)
    ordinary = [t.task for t in cases.trajectory_batches()[key]]
    degenerate = cases.degenerate_tasks(n_dims)
    mixed, where = [], {}
    for pos in range(max(len(ordinary), len(degenerate))):
        for kind, pool in (("degenerate", degenerate), ("ordinary", ordinary)):
            if pos < len(pool):
                where[kind, pos] = len(mixed)
                mixed.append(pool[pos][1] if kind == "degenerate" else pool[pos])
    res = quiet_solve(X, y, mixed, kernel=kernel, eps=eps)
    alone = quiet_solve(X, y, ordinary, kernel=kernel, eps=eps)
    for pos, (name, task) in enumerate(degenerate):
        at = where["degenerate", pos]
        rows, mean, scale, C, gamma, epsilon = task
        n, t = len(rows), y[rows]
        K = smo_ref.gram(cases.standardised(X, task), kernel, gamma)
        assert res.status[at] == audioTrainTest.SMO_CONVERGED and res.beta[at].shape == (n,), name
        if name == "all_at_C":
            assert np.array_equal(res.beta[at], np.where(t > 0, C, -C)) and res.n_sv[at] == n and res.iterations[at] >= n // 2
            alpha = np.concatenate([np.maximum(res.beta[at], 0.0), np.maximum(-res.beta[at], 0.0)])     # at +-C: one of a row's two is 0
            want = smo_ref.rho_of(alpha, ref.gradient(K, t, alpha, epsilon), ref.dual_signs(n), C)
            assert close(res.rho[at], want), (name, res.rho[at], want)
            continue
        alpha, G, rho, it, gap, status = ref.solve(K, t, C, epsilon, eps)
        assert it == 0 and res.iterations[at] == 0 and not res.beta[at].any() and res.n_sv[at] == 0, name
        assert res.gap[at] == gap and res.rho[at] == rho == smo_ref.rho_of(alpha, G, ref.dual_signs(n), C), (name, res.gap[at], gap, res.rho[at], rho)
        assert np.array_equal(res.train_pred[at], G[:n] - epsilon + t - rho), name
    for pos in range(len(ordinary)):
        at = where["ordinary", pos]
        assert res.beta[at].tobytes() == alone.beta[pos].tobytes() and res.beta[at].any()
        assert res.train_pred[at].tobytes() == alone.train_pred[pos].tobytes()
        assert res.rho[at].tobytes() == alone.rho[pos].tobytes() and res.gap[at].tobytes() == alone.gap[pos].tobytes()
        assert res.iterations[at] == alone.iterations[pos] > 0 and res.status[at] == alone.status[pos] and res.n_sv[at] == alone.n_sv[pos]


def launches_of(iterations, ipl):
    """What svr_smo_kernel's loop and smo_relaunch imply: a launch gives every live task `ipl` iterations; at the head of the loop
    the stop of a task -- converged, then max_iter -- is tested BEFORE the budget (`if (done >= budget) break` comes third), so a
    stop that falls on a budget boundary is seen by the launch that made the last iteration (no launch more); a task that stops
    at once still takes one launch.  The host relaunches while any task is below kConverged: the batch needs its slowest task's."""
    return max(max(1, -(-int(it) // ipl)) for it in iterations)


def test_max_iter_against_the_launch_budget(gpu_lib):
    """max_iter 1 .. 5 under 1, 2, 3 and 7 iterations per launch (the kFresh -> kRunning handover, a stop on and off a budget
    boundary, the launch cap max_iter / budget + 2): no error, the bytes of the default budget, the launches of the loop."""
    long, one = cases.budget_tasks()
    X, y = cases.trajectory_matrix(cases.BUDGET_DIMS)
    full = quiet_solve(X, y, [long, one], kernel="linear", eps=cases.BUDGET_EPS)
    assert full.iterations[0] > 5 and full.iterations[1] == 1 and full.n_launches == 1
    for max_iter in range(1, 6):
        want = quiet_solve(X, y, [long, one], kernel="linear", eps=cases.BUDGET_EPS, max_iter=max_iter)
        assert want.iterations.tolist() == [max_iter, 1] and want.n_launches == 1
        assert want.status.tolist() == [audioTrainTest.SMO_NOT_CONVERGED, audioTrainTest.SMO_CONVERGED]
        for ipl in (1, 2, 3, 7):
            got = quiet_solve(X, y, [long, one], kernel="linear", eps=cases.BUDGET_EPS, max_iter=max_iter, iters_per_launch=ipl)
            assert same_bytes(got, want), (max_iter, ipl)
            assert got.n_launches == launches_of(want.iterations, ipl), (max_iter, ipl, got.n_launches)


def test_a_sweep_job_does_not_depend_on_its_call(gpu_lib):
    """One call of svr_split_fit_predict holding the constant-row job (gamma exactly 1.0), jobs that differ in C alone and jobs
    with their own 'scale' gammas: every job's predictions, training predictions, gamma, iterations, status and n_sv are
    bit-identical to the same job in a call of its own."""
    call = cases.sweep_call()
    res = quiet_sweep(call.X, call.y, call.jobs, kernel="rbf", gamma=None, epsilon=cases.SWEEP_EPSILON, train_pred=True)
    assert res.gamma[call.names.index("constant")] == 1.0 and np.all(res.status == audioTrainTest.SMO_CONVERGED)
    assert len(np.unique(res.gamma)) == 5 and res.iterations[0] >= 1
    same_rows = [call.names.index(k) for k in ("C0.05", "C1", "C20")]
    assert len({res.pred[res.test_off[j]:res.test_off[j + 1]].tobytes() for j in same_rows}) == 3
    for j, job in enumerate(call.jobs):
        alone = quiet_sweep(call.X, call.y, [job], kernel="rbf", gamma=None, epsilon=cases.SWEEP_EPSILON, train_pred=True)
        pred, train_pred, its, status, n_sv = res.job(j)
        want = alone.job(0)
        assert pred.shape == (len(job[1]),) and pred.tobytes() == want[0].tobytes() and train_pred.tobytes() == want[1].tobytes(), call.names[j]
        assert (its, status, n_sv) == want[2:] and res.gamma[j] == alone.gamma[0] == ref.scale_gamma((call.X[job[0]] - job[2]) / job[3]), call.names[j]
