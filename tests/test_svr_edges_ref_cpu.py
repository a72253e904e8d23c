"""The conditions that make the inputs of tests/svr_edge_cases.py meaningful, asserted on the restatement (tests/svr_fit_ref.py)
alone.  They are no measurements of the code under test: if an input fails one, the input changes, never the condition.
tests/test_svr_edges_gpu.py runs the same inputs through svr_smo_kernel.  No GPU needed.

The mutant tests are the proof that the GPU test fails for a solver that breaks one of libsvm's rules: each mutant of
svr_fit_ref.solve (and a batch that reads task 0's epsilon or gamma for every task) differs from the restatement in what the
GPU test observes -- beta after one of the first 8 steps by more than 1e-6 C, the final iteration count, or the status.  One
mutant the issue lists cannot be told apart by anything, see test_swapped_clip_passes_are_the_same_solver."""
import functools
import warnings

import numpy as np
import pytest

import smo_edge_cases
import smo_ref
import svr_edge_cases as cases
import svr_fit_ref as ref

ALL_BRANCHES = {"A1", "A2", "A3", "A4", "B1", "B2", "B3", "B4"}
MARGIN = 1e-6                   # of max(1, max |G|): three orders above the 1e-9 the GPU test grants beta
ETA_REL = 1e-3
STEPS = 8
BETA_SEEN = 1e-6                # of C: what counts as a different beta for a mutant, three orders above the GPU test's gate
TASKS = {t.name: t for t in cases.trajectory_tasks()}


def task_gram(t, gamma=None):
    X, _ = cases.trajectory_matrix(t.n_dims)
    gamma = t.task[4] if gamma is None else gamma
    return smo_ref.gram(cases.standardised(X, t.task), t.kernel, 1.0 / t.n_dims if gamma is None else gamma)


def targets(t):
    return cases.trajectory_matrix(t.n_dims)[1][t.task[0]]


@functools.lru_cache(maxsize=None)
def traced(name):
    t = TASKS[name]
    return ref.solve_trace(task_gram(t), targets(t), t.task[3], t.task[5], t.eps)


@functools.lru_cache(maxsize=None)
def observed(name, mutant=None, epsilon=None, gamma=None):
    """What the GPU test sees of a task: (beta, iterations, status) after max_iter = 1 .. 8 and unbounded; under a mutant of the
    solver, or with another task's epsilon or gamma."""
    t = TASKS[name]
    K, y, n = task_gram(t, gamma), targets(t), len(t.task[0])
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in list(range(1, STEPS + 1)) + [10**5]:
            alpha, G, rho, it, gap, status = ref.solve(K, y, t.task[3], t.task[5] if epsilon is None else epsilon, t.eps, m, mutant=mutant)
            out.append((alpha[:n] - alpha[n:], it, status))
    return out


def told_apart(name, **kw):
    C = TASKS[name].task[3]
    for k, ((b0, it0, st0), (b1, it1, st1)) in enumerate(zip(observed(name), observed(name, **kw))):
        if (it0, st0) != (it1, st1) or (k < STEPS and not np.all(np.abs(b0 - b1) <= BETA_SEEN * C)):
            return True
    return False


def test_traced_solve_is_the_solve():
    """trace= changes nothing of what solve returns, and records one entry per iteration."""
    for t in cases.trajectory_tasks()[:8] + cases.trajectory_tasks()[-3:]:
        K, y, C, epsilon = task_gram(t), targets(t), t.task[3], t.task[5]
        plain = ref.solve(K, y, C, epsilon, t.eps)
        (alpha, G, rho, it, gap, status), trace = ref.solve_trace(K, y, C, epsilon, t.eps)
        assert alpha.tobytes() == plain[0].tobytes() and G.tobytes() == plain[1].tobytes() and (rho, it, gap, status) == plain[2:]
        assert len(trace) == it
        short, trace3 = ref.solve_trace(K, y, C, epsilon, t.eps, max_iter=min(it, 3))
        assert len(trace3) == short[3] == min(it, 3) and [(s["i"], s["j"]) for s in trace3] == [(s["i"], s["j"]) for s in trace[:3]]


def twins_of(field):
    """[(task, its twin)]: pairs of one batch that differ in the task field `field` (4: gamma, 5: epsilon) alone."""
    out = []
    for batch in cases.trajectory_batches().values():
        for a, t in enumerate(batch):
            for u in batch[a + 1:]:
                same = all(np.array_equal(t.task[f], u.task[f]) for f in range(6) if f != field)
                if same and t.task[field] != u.task[field]:
                    out.append((t, u))
    return out


def test_trajectory_set_covers_what_the_issue_asks():
    tasks = cases.trajectory_tasks()
    assert 14 <= len(tasks) <= 24
    sizes = [len(t.task[0]) for t in tasks]
    assert min(sizes) == 2 and max(sizes) == 70
    assert {t.n_dims for t in tasks} == {1, 9, 256} and {t.kernel for t in tasks} == {"linear", "rbf"}
    assert {t.task[3] for t in tasks} == {0.05, 1.0, 20.0} and {t.eps for t in tasks} == {1e-3, 1e-2, 1e-1}
    assert {t.task[5] for t in tasks} == {0.0, 0.1, 0.5}
    for n_dims in (1, 9, 256):
        assert {t.kernel for t in tasks if t.n_dims == n_dims} == {"linear", "rbf"}
    by_epsilon, by_gamma = twins_of(5), twins_of(4)
    assert len(by_epsilon) >= 2 and len(by_gamma) >= 2 and all(t.kernel == "rbf" for t, u in by_gamma)
    for t, u in by_epsilon + by_gamma:                  # and the parameter matters
        (a, *_), (b, *_) = traced(t.name)[0], traced(u.name)[0]
        n = len(t.task[0])
        assert np.max(np.abs((a[:n] - a[n:]) - (b[:n] - b[n:]))) > BETA_SEEN * t.task[3], (t.name, u.name)
    for key, batch in cases.trajectory_batches().items():
        assert len({t.name for t in batch}) == len(batch), key


@pytest.mark.parametrize("name", list(TASKS))
def test_trajectory_selections_are_decided_far_above_rounding(name):
    """Every selection of the whole run.  Against the candidates of OTHER rows: a margin of at least 1e-6 max(1, max |G|), or
    exactly 0 where the construction makes it so (in the TAU tasks, rows that are the same point).  Against the other variable of
    the chosen row, when that is a candidate too: exactly 0 at epsilon = 0 -- G[t + n] == -G[t] bit for bit, same eta: the tie
    the greatest index decides -- and at least the margin otherwise.  eta / (QD_i + QD_j) >= 1e-3 but on the designed TAU pair;
    the stopping test |gap - eps| away from rounding as well, so that the iteration count is decided.  The clips are decisions too: no
    new value comes within 1e-6 C of a bound before the clips, and after them none lies within 1e-6 C of a bound unless it is
    0 or C in any arithmetic (svr_fit_ref.solve, bound_margin).  The second rule was learned on the GPU: a task whose two
    variables had moved together met C through alpha_i - alpha_j = 0; with the kernel's fused multiply-add in the gradient they
    differed by one ulp, one stayed an ulp inside C and the run took one iteration more (reproduced on the CPU with an exact
    fma); libsvm's rules allow both, so the task left the set."""
    t = TASKS[name]
    (alpha, G, rho, it, gap, status), trace = traced(name)
    assert status == ref.STATUS_CONVERGED and it == len(trace) >= 1
    n, epsilon = len(t.task[0]), t.task[5]
    same_point = cases.same_point_rows(cases.trajectory_matrix(t.n_dims)[0], t.task)
    assert same_point.any() == t.tau
    for k, s in enumerate(trace):
        for which in "ij":
            margin, partner, row = s["margin_" + which], s["partner_" + which], s[which] % n
            assert margin >= MARGIN * s["g_scale"] or (margin == 0.0 and same_point[row]), (name, k, which, margin)
            if epsilon == 0.0:
                assert partner in (0.0, np.inf), (name, k, which, partner)
            else:
                assert partner >= MARGIN * s["g_scale"], (name, k, which, partner)
        assert abs(s["gap"] - t.eps) >= MARGIN, (name, k)
        assert s["clip_margin"] >= MARGIN and s["bound_margin"] >= MARGIN, (name, k, s["clip_margin"], s["bound_margin"])
        if s["tau"]:
            assert same_point[s["i"] % n] and same_point[s["j"] % n] and s["i"] % n != s["j"] % n, (name, k)
        else:
            assert s["eta_rel"] >= ETA_REL, (name, k, s["eta_rel"])
    assert abs(gap - t.eps) >= MARGIN or gap == 0.0


def test_epsilon_zero_tasks_tie_within_a_row():
    """At epsilon = 0 the two variables of a row tie exactly whenever both are candidates: at least three tasks meet such a tie in
    the choice of i, and three in the choice of j, within the steps after which the GPU test compares beta; the greatest index, t
    + n, is chosen.  Some state holds both alphas of a row above zero (what dual_state() of test_svr_fit_gpu.py assumes away)."""
    tie_i, tie_j, both = [], [], []
    for t in cases.trajectory_tasks():
        trace, n = traced(t.name)[1], len(t.task[0])
        if t.task[5] != 0.0:
            assert not any(s["row_tie_i"] or s["row_tie_j"] for s in trace), t.name
            continue
        for s in trace:
            assert (not s["row_tie_i"] or s["i"] >= n) and (not s["row_tie_j"] or s["j"] >= n), t.name
        if t.tau:
            continue
        tie_i += [t.name] * any(s["row_tie_i"] for s in trace[:STEPS])
        tie_j += [t.name] * any(s["row_tie_j"] for s in trace[:STEPS])
        both += [t.name] * any(s["both_above"] for s in trace)
    assert len(tie_i) >= 3 and len(tie_j) >= 3 and len(both) >= 1, (tie_i, tie_j, both)


def test_trajectory_set_reaches_every_clip_branch_and_tau():
    seen, tau_steps = set(), {}
    for t in cases.trajectory_tasks():
        trace = traced(t.name)[1]
        seen |= {b for s in trace for b in s["branches"]}
        if any(s["tau"] for s in trace):
            tau_steps[t.name] = [k for k, s in enumerate(trace) if s["tau"]]
    assert seen == ALL_BRANCHES
    assert sorted(tau_steps) == sorted(t.name for t in cases.trajectory_tasks() if t.tau) and len(tau_steps) >= 2
    for name, steps in tau_steps.items():               # on the path, not as the whole problem
        assert len(TASKS[name].task[0]) > 2 and min(steps) >= 1 and traced(name)[0][3] > max(steps) + 1, (name, steps)
    # all eight already within the steps after each of which the GPU test compares beta
    early = {b for t in cases.trajectory_tasks() for s in traced(t.name)[1][:STEPS] for b in s["branches"]}
    assert early == ALL_BRANCHES


@pytest.mark.parametrize("mutant", ["least_index", "first_order", "no_second_clip", "no_tau"])
def test_a_solver_that_breaks_a_rule_is_told_apart(mutant):
    """At least two tasks of the set tell each mutant from the restatement.  "least_index" by a tie WITHIN a row at epsilon =
    0, on at least three tasks: those tasks have no other tie (the margins above)."""
    apart = [name for name in TASKS if told_apart(name, mutant=mutant)]
    print(mutant, apart)
    assert len(apart) >= 2, (mutant, apart)
    if mutant == "least_index":
        by_row_tie = [name for name in apart if not TASKS[name].tau and TASKS[name].task[5] == 0.0]
        assert len(by_row_tie) >= 3, by_row_tie
        for name in by_row_tie:
            assert any(s["row_tie_i"] or s["row_tie_j"] for s in traced(name)[1])
    if mutant == "no_tau":
        assert all(TASKS[name].tau for name in apart)


def test_swapped_clip_passes_are_the_same_solver():
    """The issue lists "the two clip passes of each branch applied in swapped order" among the mutants to tell apart.  No input
    can: the two passes of a branch never both fire, and neither changes whether the other does.  For s_i != s_j the first pass
    needs a new value below 0 (alpha + delta < 0 <= alpha: delta < 0) and the second one above C (alpha + delta > C >= alpha:
    delta > 0); after either has fired both values lie in [0, C] (|d| <= C), so the other finds nothing.  For equal signs the
    two passes ask for delta > 0 and delta < 0 in the same way.  IEEE addition is monotone, so this holds in floating point
    too: the swapped solver returns the restatement's bits.  Asserted here on every task; the mutant that stands in for a
    wrong clip is "no_second_clip" above."""
    for name, t in TASKS.items():
        want = traced(name)[0]
        got = ref.solve(task_gram(t), targets(t), t.task[3], t.task[5], t.eps, mutant="swapped_clips")
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:], name


@pytest.mark.parametrize("field, what", [(5, "epsilon"), (4, "gamma")])
def test_a_batch_that_reads_task_0s_parameter_is_told_apart(field, what):
    """A kernel that used the epsilon (the gamma) of the first task of its batch for every task: at least two tasks tell."""
    apart = []
    for key, batch in cases.trajectory_batches().items():
        first = batch[0].task[field]
        first = 1.0 / key[0] if first is None else first
        for t in batch[1:]:
            own = 1.0 / key[0] if t.task[field] is None else t.task[field]
            if own != first and (what == "epsilon" or t.kernel == "rbf") and told_apart(t.name, **{what: first}):
                apart.append(t.name)
    print(what, apart)
    assert len(apart) >= 2, apart


def test_tie_layouts_tie_exactly():
    """Step 1 of every layout on the restatement: the margin of both selections is exactly 0 (at least 1 where the layout leaves one
    best candidate: every row is a candidate here, the others with integer values below), i is the greatest index among the rows of the greatest target and j is n + the greatest index among the tied
    best; exactly those two rows are touched, by the unclipped step (6 - 2 epsilon) / 3."""
    X, y = cases.tie_matrix()
    layouts = cases.tie_layouts()
    assert {len(lay.task[0]) for lay in layouts} == set(smo_edge_cases.TIE_ROWS)
    assert {lay.task[5] for lay in layouts} == set(cases.TIE_EPSILONS) and {kind for lay in layouts for kind in ("one", "scattered") if kind in lay.name} == {"one", "scattered"}
    for n in smo_edge_cases.TIE_ROWS:
        want = {p for p in smo_edge_cases.EDGE_POSITIONS + (n - 1,) if p < n}
        assert {lay.i for lay in layouts if len(lay.task[0]) == n} == want
        assert n < 33 or len({lay.j for lay in layouts if len(lay.task[0]) == n and "scattered" in lay.name}) >= 2
    for lay in layouts:
        rows, mean, scale, C, _, epsilon = lay.task
        n, t = len(rows), y[rows]
        (alpha, G, rho, it, gap, status), trace = ref.solve_trace(smo_ref.gram(cases.standardised(X, lay.task), "linear", 0), t, C, epsilon,
                                                                  1e-3, max_iter=1)
        s = trace[0]
        assert it == 1 and (s["i"], s["j"]) == (lay.i, lay.j), lay.name
        assert (s["margin_i"] == 0.0) if lay.n_top > 1 else (s["margin_i"] >= 1.0), lay.name
        assert (s["margin_j"] == 0.0) if lay.n_tied_j > 1 else (s["margin_j"] >= 1.0), lay.name
        assert lay.i == np.flatnonzero(t == t.max())[-1] and t[lay.j - n] == t.min()
        assert np.array_equal(np.flatnonzero(alpha), [lay.i, lay.j]) and not s["branches"] and not s["tau"]
        assert alpha[lay.i] == alpha[lay.j] == (6.0 - 2.0 * epsilon) / 3.0 < C
        if "scattered" in lay.name:                     # neither the first nor the last row of the least target
            least = np.flatnonzero(t == t.min())
            assert lay.j - n < least[-1] and (lay.n_tied_j == 1 or lay.j - n > least[0])
    assert sum(lay.n_top > 1 and lay.n_tied_j > 1 for lay in layouts) >= 0.8 * len(layouts)


@pytest.mark.parametrize("n_dims", [1, 9, 256])
def test_degenerate_tasks_have_nothing_to_solve(n_dims):
    X, y = cases.trajectory_matrix(n_dims)
    tasks = dict(cases.degenerate_tasks(n_dims))
    assert set(tasks) == set(cases.ZERO_ITERATION) | {"all_at_C"}
    assert len(tasks["one_e0"][0]) == len(tasks["one_e0.1"][0]) == 1 and (tasks["one_e0"][5], tasks["one_e0.1"][5]) == (0.0, 0.1)
    assert (tasks["equal_e0"][5], tasks["equal_e0.1"][5]) == (0.0, 0.1)
    for kernel in ("linear", "rbf"):
        for name, task in tasks.items():
            rows, mean, scale, C, gamma, epsilon = task
            n, t = len(rows), y[rows]
            alpha, G, rho, it, gap, status = ref.solve(smo_ref.gram(cases.standardised(X, task), kernel, gamma), t, C, epsilon)
            assert status == ref.STATUS_CONVERGED
            if name == "all_at_C":
                assert it >= n // 2 and np.array_equal(alpha[:n] - alpha[n:], np.where(t > 0, C, -C))
                continue
            assert it == 0 and not alpha.any(), name
            assert gap == np.max(-(epsilon - t)) + np.max(-(epsilon + t)) < 1e-3, name                # y_max - y_min - 2 epsilon
            assert abs(gap - (t.max() - t.min() - 2.0 * epsilon)) <= 1e-15
            assert rho == ref.rho_of(alpha, G, ref.dual_signs(n), C) == (np.min(epsilon - t) + np.max(-(epsilon + t))) / 2.0, name
            if name.startswith("equal"):
                assert n == cases.N_EQUAL and np.all(t == cases.EQUAL_TARGET) and abs(gap + 2.0 * epsilon) <= 1e-15
                assert epsilon > 0 or gap == 0.0


def test_sweep_call_holds_what_the_issue_asks():
    call = cases.sweep_call()
    jobs = dict(zip(call.names, call.jobs))
    train, test, mean, scale, C = jobs["constant"]
    Z = (call.X[train] - mean) / scale
    assert len(train) > 2 and not Z.any() and ref.scale_gamma(Z) == 1.0 and len(np.unique(call.y[train])) == 2
    same = [jobs[k] for k in ("C0.05", "C1", "C20")]
    assert [job[4] for job in same] == [0.05, 1.0, 20.0]
    assert all(all(np.array_equal(a, b) for a, b in zip(job[:4], same[0][:4])) for job in same)
    gammas = [ref.scale_gamma((call.X[job[0]] - job[2]) / job[3]) for job in call.jobs]
    assert len({gammas[call.names.index(k)] for k in ("C1", "own33", "own12", "own70")}) == 4
    fits = [ref.fit_job(call.X, call.y, job, "rbf", None, cases.SWEEP_EPSILON) for job in call.jobs]
    assert all(f[5] == ref.STATUS_CONVERGED for f in fits) and fits[0][7] == 1.0
    assert fits[0][4] >= 1 and len({f[4] for f in fits[1:4]}) == 3          # the constant job iterates; C moves the iteration count
