"""The conditions that make the inputs of tests/smo_edge_cases.py meaningful, asserted on the restatement (tests/smo_ref.py)
alone.  They are no measurements of the code under test: if an input fails one, the input changes, never the condition.
tests/test_smo_edges_gpu.py runs the same inputs through smo_kernel and svc_pairs_kernel.  No GPU needed."""
import functools

import numpy as np
import pytest

import smo_edge_cases as cases
import smo_ref

ALL_BRANCHES = {"A1", "A2", "A3", "A4", "B1", "B2", "B3", "B4"}
MARGIN = 1e-6                   # of max(1, max |G|): three orders above the 1e-9 the GPU test grants the alphas
ETA_REL = 1e-3


@functools.lru_cache(maxsize=None)
def traced(name):
    t = {c.name: c for c in cases.trajectory_tasks()}[name]
    X, _ = cases.trajectory_matrix(t.n_dims)
    rows, y, mean, scale, C, gamma = t.task
    K = smo_ref.gram(cases.standardised(X, t.task), t.kernel, 1.0 / t.n_dims if gamma is None else gamma)
    return smo_ref.solve_trace(K, y, C, t.eps)


def test_traced_solve_is_the_solve():
    """trace= changes nothing of what solve returns, and records one entry per iteration."""
    for t in cases.trajectory_tasks()[:6]:
        X, _ = cases.trajectory_matrix(t.n_dims)
        K = smo_ref.gram(cases.standardised(X, t.task), t.kernel, 1.0 / t.n_dims if t.task[5] is None else t.task[5])
        plain = smo_ref.solve(K, t.task[1], t.task[4], t.eps)
        (alpha, rho, it, gap, status), trace = smo_ref.solve_trace(K, t.task[1], t.task[4], t.eps)
        assert alpha.tobytes() == plain[0].tobytes() and (rho, it, gap, status) == plain[1:] and len(trace) == it
        short, trace3 = smo_ref.solve_trace(K, t.task[1], t.task[4], t.eps, max_iter=min(it, 3))
        assert len(trace3) == short[2] == min(it, 3) and [(s["i"], s["j"]) for s in trace3] == [(s["i"], s["j"]) for s in trace[:3]]


def test_trajectory_set_covers_what_the_issue_asks():
    tasks = cases.trajectory_tasks()
    assert 12 <= len(tasks) <= 20
    sizes = [len(t.task[0]) for t in tasks]
    assert min(sizes) == 2 and max(sizes) == 70
    assert {t.n_dims for t in tasks} == {1, 9, 256} and {t.kernel for t in tasks} == {"linear", "rbf"}
    assert {t.task[4] for t in tasks if not t.tau} == {0.05, 1.0, 20.0}
    gammas = [t for t in tasks if t.task[5] is not None]
    assert len(gammas) >= 2 and all(t.kernel == "rbf" and t.task[5] != 1.0 / t.n_dims for t in gammas)
    for g in gammas:                                    # its twin under the default gamma is in the same batch
        twins = [t for t in cases.trajectory_batches()[(g.n_dims, g.kernel, g.eps)]
                 if t.task[5] is None and np.array_equal(t.task[0], g.task[0]) and t.task[4] == g.task[4]]
        assert len(twins) == 1
        assert traced(twins[0].name)[0][0].tobytes() != traced(g.name)[0][0].tobytes()      # and gamma matters


@pytest.mark.parametrize("name", [t.name for t in cases.trajectory_tasks()])
def test_trajectory_selections_are_decided_far_above_rounding(name):
    """Every selection of the whole run: a margin of at least 1e-6 max(1, max |G|), or exactly 0 where the construction makes it
    so -- the choice of i at iteration 0 (alpha = 0, G = -1: every positive row has v = 1) and, in the TAU tasks, rows that
    are the same sample; eta / (QD_i + QD_j) >= 1e-3 but on the designed TAU pair; the stopping test |gap - eps| away from
    rounding as well, so that the iteration count is decided."""
    t = {c.name: c for c in cases.trajectory_tasks()}[name]
    (alpha, rho, it, gap, status), trace = traced(name)
    assert status == smo_ref.STATUS_CONVERGED and it == len(trace) >= 1
    rows = t.task[0]
    for k, s in enumerate(trace):
        for which, chosen in (("margin_i", s["i"]), ("margin_j", s["j"])):
            by_construction = (k == 0 and which == "margin_i") or (t.tau and np.count_nonzero(rows == rows[chosen]) > 1)
            assert s[which] >= MARGIN * s["g_scale"] or (s[which] == 0.0 and by_construction), (name, k, which, s[which])
        assert abs(s["gap"] - t.eps) >= MARGIN, (name, k)
        if s["tau"]:
            assert t.tau and rows[s["i"]] == rows[s["j"]], (name, k)
        else:
            assert s["eta_rel"] >= ETA_REL, (name, k, s["eta_rel"])
    assert abs(gap - t.eps) >= MARGIN or gap == 0.0


def test_trajectory_set_reaches_every_clip_branch_and_tau():
    seen, tau_rows = set(), []
    for t in cases.trajectory_tasks():
        trace = traced(t.name)[1]
        seen |= {b for s in trace for b in s["branches"]}
        if any(s["tau"] for s in trace):
            tau_rows.append(len(t.task[0]))
    assert seen == ALL_BRANCHES
    assert [t.name for t in cases.trajectory_tasks() if t.tau and not any(s["tau"] for s in traced(t.name)[1])] == []
    assert tau_rows and min(tau_rows) > 2
    # six of the eight already within the steps after each of which the GPU test compares alpha (the other two move the
    # iteration count it compares)
    early = {b for t in cases.trajectory_tasks() for s in traced(t.name)[1][:8] for b in s["branches"]}
    assert {"A1", "A3", "A4", "B1", "B2", "B3"} <= early


def test_tie_layouts_tie_exactly():
    """Step 1 of every layout on the restatement: the margin of both selections is exactly 0 (inf where the layout leaves one
    candidate), i is the greatest positive index and j the greatest index among the tied best."""
    X = cases.tie_matrix()
    layouts = cases.tie_layouts()
    assert {len(lay.task[0]) for lay in layouts} == set(cases.TIE_ROWS)
    for n in cases.TIE_ROWS:
        want = {p for p in cases.EDGE_POSITIONS + (n - 1,) if p < n}
        assert {lay.i for lay in layouts if len(lay.task[0]) == n} == want
        assert n < 33 or len({lay.j for lay in layouts if len(lay.task[0]) == n and "scattered" in lay.name}) >= 2
    for lay in layouts:
        rows, y, mean, scale, C, _ = lay.task
        (alpha, rho, it, gap, status), trace = smo_ref.solve_trace(smo_ref.gram(cases.standardised(X, lay.task), "linear", 0), y, C,
                                                                   1e-3, max_iter=1)
        s = trace[0]
        assert it == 1 and (s["i"], s["j"]) == (lay.i, lay.j), lay.name
        assert s["margin_i"] == (0.0 if lay.n_positive > 1 else np.inf), lay.name
        assert s["margin_j"] == (0.0 if lay.n_tied_j > 1 else np.inf), lay.name
        assert lay.i == np.flatnonzero(y > 0)[-1] and np.array_equal(np.flatnonzero(alpha), sorted((lay.i, lay.j)))
        assert alpha[lay.i] == alpha[lay.j] == 2.0 / 3.0 and not s["branches"]
        if "scattered" in lay.name:                     # neither the first nor the last negative row
            negatives = np.flatnonzero(y < 0)
            assert lay.j < negatives[-1] and (lay.n_tied_j == 1 or lay.j > negatives[0])
    assert sum(lay.n_positive > 1 and lay.n_tied_j > 1 for lay in layouts) >= 0.8 * len(layouts)


def test_degenerate_tasks_have_nothing_to_solve():
    for n_dims in (1, 9):
        X, _ = cases.trajectory_matrix(n_dims)
        names = [name for name, _ in cases.degenerate_tasks(n_dims)]
        assert names == ["one_plus", "one_minus", "five_plus", "five_minus", "two_plus", "two_minus"]
        for name, task in cases.degenerate_tasks(n_dims):
            rows, y, mean, scale, C, gamma = task
            assert len(rows) == {"one": 1, "two": 2, "five": 5}[name.split("_")[0]] and abs(np.sum(y)) == len(rows)
            for kernel in ("linear", "rbf"):
                alpha, rho, it, gap, status = smo_ref.solve(smo_ref.gram(cases.standardised(X, task), kernel, gamma), y, C)
                assert status == smo_ref.STATUS_CONVERGED and it == 0 and gap == 0.0 and not alpha.any()
                assert rho == (-np.inf if y[0] > 0 else np.inf)


@functools.lru_cache(maxsize=None)
def fitted(name):
    call = {c.name: c for c in cases.all_vote_calls()}[name]
    return [smo_ref.fit_job(call.X, call.labels, job, call.kernel, call.gamma) for job in call.jobs]


def _votes(dec, k):
    votes = np.zeros((dec.shape[0], k), dtype=np.int64)
    p = 0
    for a in range(k):
        for b in range(a + 1, k):
            votes[np.arange(dec.shape[0]), np.where(dec[:, p] > 0, a, b)] += 1
            p += 1
    return votes


def test_vote_calls_cover_what_the_issue_asks():
    calls = cases.vote_calls()
    ks = [len(np.unique(c.labels[c.jobs[0][0]])) for c in calls if c.name != "mixed"]
    assert ks == [2, 3, 4, 8, 9, 16, 17, 64]
    lengths = sorted({len(job[1]) for c in calls for job in c.jobs})
    assert lengths == [0, 1, 31, 32, 33, 97]
    for c in calls:
        assert 2 <= c.X.shape[1] <= 9
        values = np.unique(c.labels)
        assert np.array_equal(values, [cases.class_value(i) for i in range(len(values))]) and values[0] == 5
        for train, test, mean, scale, C in c.jobs:
            k = len(np.unique(c.labels[train]))
            if k >= 16:
                counts = np.unique(c.labels[train], return_counts=True)[1]
                assert counts.min() >= 3 and counts.max() <= 6
            if len(test) >= 31:
                assert len(np.unique(test)) < len(test) and np.isin(test, train).any() and not np.isin(test, train).all()
    mixed = calls[-1]
    ks = [len(np.unique(mixed.labels[j[0]])) for j in mixed.jobs]
    assert ks[0] == 2 and ks[2] == 9 and 2 <= ks[1] <= 9
    assert [len(j[1]) for j in mixed.jobs] == [33, 0, 31]
    assert {c.gamma for c in calls if c.kernel == "rbf"} > {None}          # an explicit gamma in the sweep as well


@pytest.mark.parametrize("name", ["k3", "k4"])
def test_tied_vote_jobs_tie(name):
    """At least 5 % of the test rows have a tied top vote, and on tied rows no decision value is within 1e-6 max|dec| of zero:
    the tie is decided by the rule, not by rounding."""
    call = {c.name: c for c in cases.vote_calls()}[name]
    assert call.tied
    for pred, dec, its, status, n_sv, classes in fitted(name):
        k = len(classes)
        votes = _votes(dec, k)
        top = votes.max(axis=1)
        tied = np.count_nonzero(votes == top[:, None], axis=1) > 1
        assert np.count_nonzero(tied) >= 0.05 * len(tied), (name, np.count_nonzero(tied), len(tied))
        assert np.min(np.abs(dec[tied])) > 1e-6 * np.max(np.abs(dec))
        assert np.all(status == smo_ref.STATUS_CONVERGED)


def test_some_tie_leaves_the_first_class_out():
    total = 0
    for name in ("k3", "k4"):
        for pred, dec, its, status, n_sv, classes in fitted(name):
            votes = _votes(dec, len(classes))
            top = votes.max(axis=1)
            tied = np.count_nonzero(votes == top[:, None], axis=1) > 1
            total += np.count_nonzero(tied & (votes[:, 0] < top))
    assert total > 0


@pytest.mark.parametrize("n", cases.TILE_ROWS)
def test_tile_jobs_end_with_every_possible_alpha_at_C(n):
    """The pair task has n rows, the first class the larger where n is odd.  An even task ends with every alpha at C.  In an
    odd one sum y alpha = 0 forbids that (the classes differ by one row): there every row of the second class is at C --
    they are the last rows of the task, so the last tile, full or partial, holds support vectors -- and the first class
    carries the same sum."""
    call = {c.name: c for c in cases.tile_calls()}["tile%d" % n]
    train, test, mean, scale, C = call.jobs[0]
    classes, tasks = smo_ref.pair_tasks(call.labels, train)
    a, b, rows, y = tasks[0]
    assert len(tasks) == 1 and len(rows) == n and np.count_nonzero(y < 0) == n // 2 and np.all(np.diff(y) <= 0)
    gamma = 1.0 / call.X.shape[1]
    alpha, rho, it, gap, status = smo_ref.solve(smo_ref.gram((call.X[rows] - mean) / scale, call.kernel, gamma), y, C)
    assert status == smo_ref.STATUS_CONVERGED
    assert np.all(alpha[y < 0] == C)
    if n % 2 == 0:
        assert np.all(alpha == C)
    else:
        assert abs(np.sum(alpha[y > 0]) - (n // 2) * C) <= 1e-12 * C and np.count_nonzero(alpha[y > 0] == C) >= n // 2 - 1
    assert alpha[-1] == C and np.count_nonzero(alpha[16 * ((n - 1) // 16):]) >= 1
    assert fitted(call.name)[0][4][0] == np.count_nonzero(alpha)


def test_exact_zero_job_is_exactly_zero():
    for call in cases.zero_calls():
        train, test, mean, scale, C = call.jobs[0]
        classes, tasks = smo_ref.pair_tasks(call.labels, train)
        a, b, rows, y = tasks[0]
        alpha, rho, it, gap, status = smo_ref.solve(smo_ref.gram(call.X[rows], "linear", 0), y, C)
        assert alpha.tolist() == [0.5, 0.5] and rho == 0.0 and status == smo_ref.STATUS_CONVERGED
        pred, dec, its, st, n_sv, classes = fitted(call.name)[0]
        assert dec.shape == (1, 1) and dec[0, 0] == 0.0 and pred.tolist() == [1]


def test_65_classes_are_refused_before_any_device_work():
    """kMaxClasses is 64: the library's 'unsupported' for a job of 65 classes comes from the host-side task builder, with no
    device call before it (this file runs without a GPU)."""
    from pyaudioanalysis_amd import audioTrainTest
    X = np.arange(130, dtype=np.float64).reshape(130, 1)
    labels = np.arange(130) % 65
    job = (np.arange(130), np.array([0, 1]), np.zeros(1), np.ones(1), 1.0)
    with pytest.raises(NotImplementedError, match="64"):
        audioTrainTest.svm_split_fit_predict(X, labels, [job])
