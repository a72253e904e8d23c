"""GPU checks of the C-SVC solver's resident kernel matrices (DESIGN K23: smo_cached_kernel over the matrices that
svr_standardise_kernel / svr_gram_kernel form for the GROUPS of a call, through paa_smo_tasks_cached_f64,
paa_svc_fit_splits_cached_f64, paa_svc_fit_proba_cached_f64 and paa_silence_batch_*_cached) and of what is built on them.  The
yardstick throughout is kernel_cache="none", the recomputing solver, itself pinned by tests/test_smo_bits_gpu.py and the goldens;
the gate is byte equality of every output: no tolerance applies.  The inputs are tests/svc_cache_cases.py's (their sizes are
asserted on the CPU in tests/test_svc_cache_cpu.py) and tests/smo_edge_cases.py's."""
import contextlib
import functools
import io
import warnings

import numpy as np
import pytest

import onset_ref
import smo_edge_cases as edges
import svc_cache_cases as cases
import train_ref
from pyaudioanalysis_amd import audioSegmentation as aS, audioTrainTest as aT
from test_platt_cpu import golden_cases

pytestmark = pytest.mark.gpu

GiB = 1 << 30


def solve(*args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return aT.smo_solve(*args, **kw)


def fields(res, t):
    """Every output of task t as bytes and integers (n_sv is the count of non-zero alpha_y: smo_solve returns no more)."""
    return (res.alpha_y[t].tobytes(), res.rho[t].tobytes(), res.gap[t].tobytes(), int(res.iterations[t]), int(res.status[t]),
            int(np.count_nonzero(res.alpha_y[t])))


def same(got, want, names=None):
    assert len(got.rho) == len(want.rho)
    for t in range(len(want.rho)):
        assert fields(got, t) == fields(want, t), (t if names is None else names[t], got.iterations[t], want.iterations[t])


@functools.lru_cache(maxsize=None)
def uncached(n_dims, kernel):
    """The recomputing solver's results for mixed_batch(n_dims): computed once, shared, never changed."""
    X, tasks, groups, names = cases.mixed_batch(n_dims)
    res = solve(X, tasks, kernel=kernel, eps=cases.EPS)
    assert not res.cached.any()
    return res


def launches_of(iterations, ipl):
    """tests/test_smo_edges_gpu.py's: what the relaunch loop implies for one set of tasks that run together."""
    return max(max(1, -(-int(it) // ipl)) for it in iterations)


# ---------------------------------------------------------------------------------------------------------------------
# the solver alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
@pytest.mark.parametrize("n_dims", cases.DIMS)
def test_the_cached_solver_is_byte_equal_to_the_recomputing_one(gpu_lib, n_dims, kernel):
    X, tasks, groups, names = cases.mixed_batch(n_dims)
    want = uncached(n_dims, kernel)
    got = solve(X, tasks, kernel=kernel, eps=cases.EPS, kernel_cache="gram", groups=groups)
    assert got.cached.dtype == bool and got.cached.all() and got.n_launches == want.n_launches
    same(got, want, names)
    print("%s %d dims: iterations %s" % (kernel, n_dims, dict(zip(names, got.iterations.tolist()))))
    assert got.iterations.max() > 100 and got.iterations[names.index("size513")] > 0
    # every task its own group: the same bytes
    own = solve(X, tasks, kernel=kernel, eps=cases.EPS, kernel_cache="gram")
    assert own.cached.all()
    same(own, want, names)


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_a_cached_task_does_not_depend_on_batch_group_budget_or_launches(gpu_lib, kernel):
    X, tasks, groups, names = cases.mixed_batch(9)
    want = uncached(9, kernel)
    for name in ("size257", "fold3", "three_02"):
        t = names.index(name)
        alone = solve(X, [tasks[t]], kernel=kernel, eps=cases.EPS, kernel_cache="gram")
        assert alone.cached.all() and fields(alone, 0) == fields(want, t), name
        mates = [k for k in range(len(tasks)) if groups[k] == groups[t]]
        assert (len(mates) > 1) == (name != "size257")
        for ipl, budget in ((0, None), (7, None), (64, cases.matrix_bytes(600)), (0, 8)):
            picked = sorted(set(mates + [0, 3]))
            res = solve(X, [tasks[k] for k in picked], kernel=kernel, eps=cases.EPS, kernel_cache="gram", groups=groups[picked],
                        iters_per_launch=ipl, cache_bytes=budget)
            assert fields(res, picked.index(t)) == fields(want, t), (name, ipl, budget)
            assert res.cached[picked.index(t)] == (budget != 8)
    # the whole batch under three launch budgets
    launches = []
    for ipl in (4, 32, 0):
        got = solve(X, tasks, kernel=kernel, eps=cases.EPS, kernel_cache="gram", groups=groups, iters_per_launch=ipl)
        same(got, want, names)
        launches.append(got.n_launches)
    assert launches[0] > launches[1] > launches[2]
    assert launches[0] == launches_of(want.iterations, 4) and launches[1] == launches_of(want.iterations, 32)


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_chunking_keeps_every_byte_and_reports_what_the_layout_implies(gpu_lib, kernel):
    X, tasks, groups, names = cases.mixed_batch(9)
    want = uncached(9, kernel)
    rows = [task[0] for task in tasks]
    group_of, group_rows, pos, _ = aT.smo_cache_layout(rows, groups, 1)
    sizes = [cases.matrix_bytes(len(r)) for r in group_rows]
    total, largest = sum(sizes), max(sizes)
    assert sizes.index(largest) not in (0, len(sizes) - 1)            # the largest group is in the middle of the call
    seen = set()
    for budget in (total, total - 1, largest, largest - 1, 8):
        chunk = aT.smo_cache_layout(rows, groups, budget)[3]
        got = solve(X, tasks, kernel=kernel, eps=cases.EPS, kernel_cache="gram", groups=groups, cache_bytes=budget, iters_per_launch=64)
        assert np.array_equal(got.cached, chunk[group_of] >= 0), budget
        same(got, want, names)
        # the launches: the uncached tasks run together, then every chunk's tasks
        sets = [np.flatnonzero(chunk[group_of] == ch) for ch in range(-1, chunk.max() + 1)]
        assert got.n_launches == sum(launches_of(want.iterations[s], 64) for s in sets if len(s)), budget
        seen.add((int(chunk.max()) + 1, int(np.count_nonzero(chunk < 0))))
    # one chunk; two chunks; one group per chunk where two do not fit together; the largest group left out in the middle; one-row groups only
    assert (1, 0) in seen and (2, 0) in seen and len(seen) == 5
    assert aT.smo_cache_layout(rows, groups, largest - 1)[3][sizes.index(largest)] == -1
    assert np.count_nonzero(aT.smo_cache_layout(rows, groups, 8)[3] >= 0) == 1
    # one group per chunk: 255, 256 and 257 rows under the budget of the largest of them
    picked = [names.index("size%d" % n) for n in (255, 256, 257)]
    assert aT.smo_cache_layout([rows[k] for k in picked], None, cases.matrix_bytes(257))[3].tolist() == [0, 1, 2]
    got = solve(X, [tasks[k] for k in picked], kernel=kernel, eps=cases.EPS, kernel_cache="gram", cache_bytes=cases.matrix_bytes(257))
    assert got.cached.all() and got.n_launches == sum(launches_of(want.iterations[k:k + 1], 1024) for k in picked)
    for at, k in enumerate(picked):
        assert fields(got, at) == fields(want, k), names[k]


def test_two_groups_with_different_gammas_read_their_own_matrices(gpu_lib):
    X, tasks, groups, names = cases.mixed_batch(9)
    want = uncached(9, "rbf")
    a, b = names.index("gamma_a0"), names.index("gamma_b0")
    assert fields(want, a) != fields(want, b) and tasks[a][0].tobytes() == tasks[b][0].tobytes()
    picked = [names.index(n) for n in ("gamma_a0", "gamma_a1", "gamma_b0", "gamma_b1")]
    got = solve(X, [tasks[k] for k in picked], kernel="rbf", eps=cases.EPS, kernel_cache="gram", groups=groups[picked])
    for at, k in enumerate(picked):
        assert fields(got, at) == fields(want, k), names[k]
    # a group's matrix alone is svr_kernel_matrix's over the group's row list: one per gamma
    rows = aT.smo_cache_layout([tasks[k][0] for k in picked], groups[picked], GiB)[1]
    mats = aT.svr_kernel_matrix(X, [(rows[g], tasks[picked[2 * g]][2], tasks[picked[2 * g]][3], tasks[picked[2 * g]][5]) for g in range(2)], "rbf")
    assert mats[0].shape == (60, 60) and mats[0].tobytes() != mats[1].tobytes()
    # one group for tasks of two gammas is refused, naming the tasks
    with pytest.raises(ValueError, match="tasks 0 and 2.*gamma"):
        solve(X, [tasks[k] for k in picked], kernel="rbf", kernel_cache="gram", groups=[0, 0, 0, 0])


@pytest.mark.parametrize("key", list(edges.trajectory_batches()), ids=lambda k: "d%d_%s_eps%g" % k)
def test_the_trajectory_tasks_under_the_cache(gpu_lib, key):
    """The clip branches, the TAU path (two rows of one sample: one matrix row) and the pairs that differ in gamma alone, after
    each of the first steps and at the end."""
    n_dims, kernel, eps = key
    batch = [t.task for t in edges.trajectory_batches()[key]]
    X, _ = edges.trajectory_matrix(n_dims)
    for m in (1, 2, 3, 5, 8, 10**7):
        want = solve(X, batch, kernel=kernel, eps=eps, max_iter=m)
        got = solve(X, batch, kernel=kernel, eps=eps, max_iter=m, kernel_cache="gram")
        assert got.cached.all() and got.n_launches == want.n_launches
        same(got, want)


def test_exact_ties_under_the_cache(gpu_lib):
    """One step on every tie layout (ties on group, wave and stride edges): every task its own group, then all of them one group
    over the 82 samples -- position lists with many repeats."""
    X = edges.tie_matrix()
    tasks = [lay.task for lay in edges.tie_layouts()]
    want = solve(X, tasks, kernel="linear", max_iter=1)
    for groups in (None, np.zeros(len(tasks), dtype=np.int32)):
        got = solve(X, tasks, kernel="linear", max_iter=1, kernel_cache="gram", groups=groups)
        assert got.cached.all()
        same(got, want, [lay.name for lay in edges.tie_layouts()])
    for pos, lay in enumerate(edges.tie_layouts()):
        assert np.flatnonzero(want.alpha_y[pos]).tolist() == sorted((lay.i, lay.j)), lay.name


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
@pytest.mark.parametrize("n_dims", [1, 9])
def test_degenerate_tasks_under_the_cache(gpu_lib, n_dims, kernel):
    X, _ = edges.trajectory_matrix(n_dims)
    ordinary = [t.task for t in edges.trajectory_tasks() if t.n_dims == n_dims and t.kernel == kernel]
    mixed = [task for name, task in edges.degenerate_tasks(n_dims)] + ordinary
    want = solve(X, mixed, kernel=kernel)
    got = solve(X, mixed, kernel=kernel, kernel_cache="gram")
    assert got.cached.all()
    same(got, want)
    assert np.isinf(want.rho[:6]).all() and not want.iterations[:6].any()


def test_max_iter_against_the_launch_budget_per_chunk(gpu_lib):
    by_name = {t.name: t for t in edges.trajectory_tasks()}
    long, two = by_name["d9_linear_n70_C0.05_s11"], by_name["d9_linear_n2_C1_s0"]
    X, _ = edges.trajectory_matrix(9)
    for max_iter in range(1, 6):
        want = solve(X, [long.task, two.task], kernel="linear", max_iter=max_iter)
        assert want.iterations.tolist() == [max_iter, 1]
        for ipl in (1, 2, 3, 7):
            one = solve(X, [long.task, two.task], kernel="linear", max_iter=max_iter, iters_per_launch=ipl, kernel_cache="gram")
            same(one, want)
            assert one.cached.all() and one.n_launches == launches_of(want.iterations, ipl), (max_iter, ipl)
            # a budget of the larger matrix alone: two chunks, each with its own launches
            cut = solve(X, [long.task, two.task], kernel="linear", max_iter=max_iter, iters_per_launch=ipl, kernel_cache="gram",
                        cache_bytes=cases.matrix_bytes(70))
            same(cut, want)
            assert cut.cached.all() and cut.n_launches == launches_of(want.iterations[:1], ipl) + launches_of(want.iterations[1:], ipl)


def test_offsets_beyond_4_gib(gpu_lib):
    """Nine groups of 8192 rows x 1 dim under a budget of 5 GiB: one chunk of 4.5 GiB, so the last group's matrix begins at byte
    offset 4 GiB; every group a task over all its rows and one over a permuted half; three iterations each."""
    X, tasks, groups = cases.big_groups()
    want = solve(X, tasks, kernel="rbf", eps=cases.EPS, max_iter=3)
    got = solve(X, tasks, kernel="rbf", eps=cases.EPS, max_iter=3, kernel_cache="gram", groups=groups, cache_bytes=5 * GiB)
    assert got.cached.all() and not want.cached.any()
    assert np.all(got.iterations == 3) and np.all(got.status == aT.SMO_NOT_CONVERGED)
    same(got, want)
    for t in range(len(tasks)):
        assert 2 <= np.count_nonzero(got.alpha_y[t]) <= 6


# ---------------------------------------------------------------------------------------------------------------------
# built on the solver
# ---------------------------------------------------------------------------------------------------------------------
VOTE_NAMES = ("k2", "k3", "k9", "mixed", "tile33", "zero_d9")


@pytest.mark.parametrize("name", VOTE_NAMES)
def test_the_sweep_returns_what_it_returns_without_the_cache(gpu_lib, name):
    c = {v.name: v for v in edges.all_vote_calls()}[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = aT.svm_split_fit_predict(c.X, c.labels, c.jobs, kernel=c.kernel, gamma=c.gamma, decision=True)
        got = aT.svm_split_fit_predict(c.X, c.labels, c.jobs, kernel=c.kernel, gamma=c.gamma, decision=True, kernel_cache="gram")
        part = aT.svm_split_fit_predict(c.X, c.labels, c.jobs, kernel=c.kernel, gamma=c.gamma, decision=True, kernel_cache="gram",
                                        cache_bytes=cases.matrix_bytes(len(c.jobs[0][0])))
    assert got.cached.all() and not want.cached.any() and part.cached[0]
    for res in (got, part):
        assert res.label.tobytes() == want.label.tobytes() and res.decision.tobytes() == want.decision.tobytes()
        assert res.iterations.tobytes() == want.iterations.tobytes() and res.status.tobytes() == want.status.tobytes()
        assert res.n_sv.tobytes() == want.n_sv.tobytes()
    assert got.n_launches == want.n_launches


PROBA_CASES = [c for c in golden_cases("platt_small") if c["name"].startswith(("two_classes", "three_classes"))]


def proba_fields(res):
    return ([a.tobytes() for a in res.alpha_y], res.rho.tobytes(), res.prob_a.tobytes(), res.prob_b.tobytes(), res.n_sv.tobytes(),
            res.iterations.tobytes(), res.status.tobytes(), res.sigmoid_iterations.tobytes(), res.sigmoid_stop.tobytes(),
            None if res.cv_dec is None else [a.tobytes() for a in res.cv_dec])


@pytest.mark.parametrize("case", PROBA_CASES, ids=lambda c: c["name"])
def test_fit_proba_returns_what_it_returns_without_the_cache(gpu_lib, case):
    c = case
    kw = dict(kernel=c["kernel"], seeds=int(c["seed"]), return_cv=True)
    want = aT.svc_fit_proba(c["X"], c["labels"], [c["job"]], **kw)
    got = aT.svc_fit_proba(c["X"], c["labels"], [c["job"]], kernel_cache="gram", **kw)
    assert got.cached.tolist() == [True] and want.cached.tolist() == [False]
    assert proba_fields(got) == proba_fields(want) and len(want.classes[0]) in (2, 3)
    # two jobs with their own seeds, the second without room for its matrix
    n = len(c["job"][0])
    two = aT.svc_fit_proba(c["X"], c["labels"], [c["job"], c["job"][:3] + (0.5 * c["job"][3],)], kernel_cache="gram",
                           cache_bytes=cases.matrix_bytes(n), iters_per_launch=50, **dict(kw, seeds=[int(c["seed"]), 5]))
    assert two.cached.tolist() == [True, True]
    half = len(want.rho)
    assert [a.tobytes() for a in two.alpha_y[:half]] == proba_fields(want)[0] and two.prob_a[:half].tobytes() == want.prob_a.tobytes()
    assert [a.tobytes() for a in two.cv_dec[:half]] == proba_fields(want)[9]


@pytest.mark.parametrize("case", PROBA_CASES, ids=lambda c: c["name"])
def test_train_svm_device_and_its_scikit_learn_model(gpu_lib, case):
    pytest.importorskip("sklearn")
    c = case
    Z, Zq = (c["X"][c["train_idx"]] - c["mean"]) / c["scale"], (c["X"][c["test_idx"]] - c["mean"]) / c["scale"]
    y = 10.0 * c["labels"][c["train_idx"]] + 3.0
    models = [aT.train_svm_device(Z, y, float(c["C"]), c["kernel"], random_state=int(c["random_state"]), **kw)
              for kw in (dict(), dict(kernel_cache="gram"), dict(kernel_cache="gram", cache_bytes=64))]
    assert [bool(m.fit_result.cached[0]) for m in models] == [False, True, False]
    svcs = [aT.to_sklearn_svc(m) for m in models]
    for m, svc in zip(models[1:], svcs[1:]):
        for name in ("support_", "support_vectors_", "_dual_coef_", "_intercept_", "probA_", "probB_", "n_support_"):
            assert np.asarray(getattr(m, name)).tobytes() == np.asarray(getattr(models[0], name)).tobytes(), name
        assert svc.predict(Zq).tobytes() == svcs[0].predict(Zq).tobytes()
        assert svc.predict_proba(Zq).tobytes() == svcs[0].predict_proba(Zq).tobytes()


def _run(fn, *args, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = fn(*args, **kw)
    return ret, out.getvalue()


@pytest.mark.parametrize("kind", ["svm", "svm_rbf"])
def test_evaluate_classifier_returns_what_it_returns_without_the_cache(gpu_lib, kind):
    pytest.importorskip("sklearn")
    feats = train_ref.class_features((100, 80, 60), 20, seed=31, spread=2.5)
    names, params, n_exp, pct = ["a", "b", "c"], [0.0001, 1.0], 3, 0.75
    runs = []
    for kw in (dict(), dict(kernel_cache="gram"), dict(kernel_cache="gram", cache_bytes=cases.matrix_bytes(180) + 8)):
        np.random.seed(10)
        runs.append(_run(aT.evaluate_classifier_full, feats, names, kind, params, 0, None, n_exp=n_exp, train_percentage=pct,
                         svm_fit="device", **kw))
    for (best, cms, preds), text in runs[1:]:
        assert best == runs[0][0][0] and text == runs[0][1] and preds == runs[0][0][2]
        assert np.array(cms).tobytes() == np.array(runs[0][0][1]).tobytes()
    assert "best Acc" in runs[0][1]


@pytest.mark.parametrize("kind", ["svm", "svm_rbf"])
def test_extract_features_and_train_writes_the_same_model_file(gpu_lib, tmp_path, kind):
    pytest.importorskip("sklearn")
    from test_train_gpu import _write_dir
    g = train_ref.load_golden("train_dir_small")
    paths = _write_dir(g, str(tmp_path))
    files = []
    for tag, kw in (("none", dict()), ("gram", dict(kernel_cache="gram"))):
        model = str(tmp_path / ("model_%s_%s" % (kind, tag)))
        np.random.seed(int(g["seed"]))
        _run(aT.extract_features_and_train, paths, float(g["mid_window"]), float(g["mid_step"]), float(g["short_window"]),
             float(g["short_step"]), kind, model, svm_fit="device", final_fit="device", **kw)
        files.append((open(model, "rb").read(), open(model + "MEANS", "rb").read()))
    assert files[0] == files[1] and len(files[0][0]) > 1000


DETAIL_KEYS = ("quiet_idx", "loud_idx", "quiet_limit", "loud_limit", "mean", "scale", "seed", "alpha_y", "rho", "prob_a", "prob_b", "n_sv",
               "status", "iterations", "sigmoid_iterations", "sigmoid_stop", "raw_prob", "prob", "threshold", "active")


def test_silence_removal_returns_what_it_returns_without_the_cache(gpu_lib):
    clips = [onset_ref.burst_clip(0), onset_ref.burst_clip(1)]
    args = (onset_ref.FS, 0.02, 0.02, 0.2, 0.4)
    want_segs, want = aS.silence_removal_batch(clips, *args, random_state=3, return_details=True)
    assert not any(d["cached"] for d in want)
    for kw in (dict(), dict(cache_bytes=cases.matrix_bytes(max(len(d["alpha_y"]) for d in want)))):
        segs, got = aS.silence_removal_batch(clips, *args, random_state=3, return_details=True, kernel_cache="gram", **kw)
        assert segs == want_segs and all(d["cached"] for d in got)
        for a, b in zip(got, want):
            for k in DETAIL_KEYS:
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert all(d["iterations"][0] > 0 and d["status"][0] == aT.SMO_CONVERGED and np.count_nonzero(d["iterations"][1:]) >= 4 for d in want)
    # the single call: the same segments, and the batch's
    for c, clip in enumerate(clips):
        one = [aS.silence_removal(clip, *args, svm_fit="device", random_state=11, **kw)
               for kw in (dict(), dict(kernel_cache="gram"))]
        assert one[0] == one[1] and len(one[0]) >= 1
    # the fit of the single call, field by field
    from pyaudioanalysis_amd import ShortTermFeatures as stf
    st, _ = stf.feature_extraction(clips[0], onset_ref.FS, 0.02 * onset_ref.FS, 0.02 * onset_ref.FS)
    quiet, loud = aS._energy_extremes(st)
    fits = [aS._train_onset_svm_device(quiet.T, loud.T, 11, *extra)[0] for extra in ((), ("gram", None))]
    assert fits[1].fit_result.cached.all() and proba_fields(fits[0].fit_result) == proba_fields(fits[1].fit_result)
