#!/usr/bin/env python3
"""Write tests/golden/smo_parent_bits.npz: every output of smo_kernel (paa_smo_tasks_f64), svr_smo_kernel (paa_svr_tasks_f64) and
svr_smo_cached_kernel (paa_svr_tasks_cached_f64) on small inputs, bit for bit, from the build BEFORE the three solvers were put on
the shared core of kernels_smo_core.hpp.

An iteration of these kernels reads nothing but (alpha, G), every selection is exact and every sum has a fixed order, so a build that
moves the two-variable update, calculate_rho or the set-up of a task into shared pieces must reproduce every output exactly -- also
which multiplies and adds the compiler fuses.  tests/test_smo_bits_gpu.py runs the calls below on the library under test, under the
launch budgets 1, 7 and the default, and asserts np.array_equal.

The calls: the trajectory and degenerate tables of tests/smo_edge_cases.py and tests/svr_edge_cases.py, the budget tasks under a
max_iter that stops the long one, and tasks at the ownership edges (a group owns rows modulo 32, a thread of the cached kernel rows
modulo 256) under a small and a large C, several tasks of different n in one call, every one stopped at SIZE_MAX_ITER at the latest.
coverage() states, on the restatements of tests/smo_ref.py and tests/svr_fit_ref.py alone, that the calls reach every clip of the
update, the clamp of eta, both formulas of rho and both stops.

    PAA_HIP_LIBRARY=<the parent build's libpaa_hip.so> python scripts/make_smo_bits_golden.py     # on the GPU, once
"""
import argparse
import collections
import functools
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "smo_parent_bits.npz")
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import smo_edge_cases  # noqa: E402
import smo_ref  # noqa: E402
import svr_edge_cases  # noqa: E402
import svr_fit_ref  # noqa: E402

BUDGETS = (1, 7, 0)             # iterations per launch; 0: the library's default
SIZE_SAMPLES = 320
SIZE_MAX_ITER = 300
SIZE_EPS = 1e-3
C_SMALL, C_LARGE = 0.05, 20.0
SVR_SIZE_ROWS = (1, 2, 31, 32, 33, 255, 256, 257, 300)
SVC_SIZE_ROWS = (2, 31, 32, 33, 257)
# (n_dims, kernel, row counts of the call's tasks): task k of a call takes C_SMALL when k + (kernel is rbf) is even, else C_LARGE
SVR_SIZE_CALLS = (
    (8, "linear", SVR_SIZE_ROWS),
    (9, "rbf", SVR_SIZE_ROWS),
    (34, "linear", (256, 2, 32)),
    (34, "rbf", (300, 33, 257)),
    (1, "linear", (300, 1, 31)),
    (1, "rbf", (255, 32)),
    (256, "linear", (2, 33)),
    (256, "rbf", (31, 1)),
)
SVC_SIZE_CALLS = (
    (8, "linear", SVC_SIZE_ROWS),
    (9, "rbf", SVC_SIZE_ROWS),
    (34, "linear", (257, 2)),
    (34, "rbf", (33, 32)),
    (1, "linear", (31, 257)),
    (1, "rbf", (32, 2)),
    (256, "linear", (2, 33)),
    (256, "rbf", (31, 2)),
)
BUDGET_MAX_ITER = 10            # of the budget tasks: the long one stops at max_iter, the short one converges first

# one call of a solver entry point: tasks as audioTrainTest.smo_solve / svr_solve take them (y: None for C-SVC)
Call = collections.namedtuple("Call", "name family X y tasks kernel eps max_iter")
SVC_OUTPUTS = ("alpha_y", "rho", "gap", "iterations", "status")
SVR_OUTPUTS = ("beta", "rho", "gap", "iterations", "status", "n_sv", "train_pred")


@functools.lru_cache(maxsize=None)
def size_matrix(n_dims):
    """(X [SIZE_SAMPLES][n_dims], y, signs): Gaussian samples, a target that is a smooth function of one direction plus noise,
    and its sign about the median as the class.  Read-only."""
    rng = np.random.default_rng(1300 + n_dims)
    X = rng.standard_normal((SIZE_SAMPLES, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    w = rng.standard_normal(n_dims) / np.sqrt(n_dims)
    y = np.tanh(X @ w - np.median(X @ w)) + 0.4 * rng.standard_normal(SIZE_SAMPLES)
    signs = np.where(y > np.median(y), 1.0, -1.0)
    for a in (X, y, signs):
        a.setflags(write=False)
    return X, y, signs


def _size_tasks(n_dims, kernel, counts, svc):
    X, y, signs = size_matrix(n_dims)
    rng = np.random.default_rng(77 * n_dims + (kernel == "rbf"))
    tasks = []
    for k, n in enumerate(counts):
        rows = rng.permutation(SIZE_SAMPLES)[:n]
        if svc and abs(signs[rows].sum()) == n:         # a C-SVC task holds both signs
            rows[-1] = np.flatnonzero(signs != signs[rows[0]])[0]
        src = X[rows] if n > 3 else X
        mean, scale = src.mean(axis=0), src.std(axis=0)
        C = C_SMALL if (k + (kernel == "rbf")) % 2 == 0 else C_LARGE
        tasks.append((rows, signs[rows], mean, scale, C, None) if svc else (rows, mean, scale, C, None, 0.1 if k % 3 else 0.0))
    return tasks


@functools.lru_cache(maxsize=None)
def calls():
    """[Call], C-SVC first."""
    out = []
    for (n_dims, kernel, eps), batch in smo_edge_cases.trajectory_batches().items():
        X, _ = smo_edge_cases.trajectory_matrix(n_dims)
        out.append(Call("svc_path_d%d_%s_eps%g" % (n_dims, kernel, eps), "svc", X, None, [t.task for t in batch], kernel, eps, 10**7))
    for n_dims, kernel in ((1, "rbf"), (9, "linear")):
        X, _ = smo_edge_cases.trajectory_matrix(n_dims)
        tasks = [task for _, task in smo_edge_cases.degenerate_tasks(n_dims)]
        out.append(Call("svc_degenerate_d%d_%s" % (n_dims, kernel), "svc", X, None, tasks, kernel, 1e-3, 10**7))
    for n_dims, kernel, counts in SVC_SIZE_CALLS:
        out.append(Call("svc_size_d%d_%s" % (n_dims, kernel), "svc", size_matrix(n_dims)[0], None, _size_tasks(n_dims, kernel, counts, True),
                        kernel, SIZE_EPS, SIZE_MAX_ITER))
    for (n_dims, kernel, eps), batch in svr_edge_cases.trajectory_batches().items():
        X, y = svr_edge_cases.trajectory_matrix(n_dims)
        out.append(Call("svr_path_d%d_%s_eps%g" % (n_dims, kernel, eps), "svr", X, y, [t.task for t in batch], kernel, eps, 10**7))
    for n_dims, kernel in ((1, "linear"), (9, "rbf")):
        X, y = svr_edge_cases.trajectory_matrix(n_dims)
        tasks = [task for _, task in svr_edge_cases.degenerate_tasks(n_dims)]
        out.append(Call("svr_degenerate_d%d_%s" % (n_dims, kernel), "svr", X, y, tasks, kernel, 1e-3, 10**7))
    X, y = svr_edge_cases.trajectory_matrix(svr_edge_cases.BUDGET_DIMS)
    out.append(Call("svr_budget", "svr", X, y, list(svr_edge_cases.budget_tasks()), "linear", svr_edge_cases.BUDGET_EPS, BUDGET_MAX_ITER))
    for n_dims, kernel, counts in SVR_SIZE_CALLS:
        X, y, _ = size_matrix(n_dims)
        out.append(Call("svr_size_d%d_%s" % (n_dims, kernel), "svr", X, y, _size_tasks(n_dims, kernel, counts, False), kernel, SIZE_EPS,
                        SIZE_MAX_ITER))
    return out


def entry_points(call):
    """The entry points a call goes through: (suffix of its keys, keyword arguments of the solve)."""
    return (("", {}),) if call.family == "svc" else (("", {}), ("_cached", {"kernel_cache": "gram"}))


def run(call, budget, **kw):
    """{output: array} of one call on the library in use; the per-task arrays are joined in task order."""
    from pyaudioanalysis_amd import audioTrainTest as aT
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # the tasks that stop at max_iter
        if call.family == "svc":
            res = aT.smo_solve(call.X, call.tasks, kernel=call.kernel, eps=call.eps, max_iter=call.max_iter, iters_per_launch=budget)
            names = SVC_OUTPUTS
        else:
            res = aT.svr_solve(call.X, call.y, call.tasks, kernel=call.kernel, eps=call.eps, max_iter=call.max_iter,
                               iters_per_launch=budget, **kw)
            names = SVR_OUTPUTS
            if kw:
                assert np.all(res.cached), call.name
    out = {}
    for name in names:
        v = getattr(res, name)
        out[name] = np.concatenate(v) if isinstance(v, list) else np.asarray(v)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what the calls reach, on the restatements alone (no device)
# ---------------------------------------------------------------------------------------------------------------------
CLIPS = ("A1", "A2", "A3", "A4", "B1", "B2", "B3", "B4")
Coverage = collections.namedtuple("Coverage", "clips unclipped tau rho stops rows dims kernels Cs tasks_per_call")


@functools.lru_cache(maxsize=None)
def coverage():
    """Coverage of calls(): the clips that fire; the branches ("A": opposite signs, "B": equal signs) with an unclipped step;
    whether eta is clamped; the formulas of rho at a stop ("free", "bounds"); the stops; per family the row counts, and the dims,
    kernels, values of C and numbers of tasks in a call."""
    clips, unclipped, rho, stops = set(), set(), set(), set()
    tau = False
    rows, dims, kernels, Cs, per_call = {"svc": set(), "svr": set()}, set(), set(), set(), set()
    for call in calls():
        n_dims = call.X.shape[1]
        dims.add(n_dims)
        kernels.add((call.family, call.kernel))
        per_call.add(len(call.tasks))
        for task in call.tasks:
            trace = []
            if call.family == "svc":
                idx, signs, mean, scale, C, gamma = task
                K = smo_ref.gram((call.X[idx] - mean) / scale, call.kernel, 1.0 / n_dims if gamma is None else gamma)
                alpha, _, _, _, status = smo_ref.solve(K, signs, C, call.eps, call.max_iter, trace)
                opposite = lambda s: signs[s["i"]] != signs[s["j"]]
            else:
                idx, mean, scale, C, gamma, epsilon = task
                n = len(idx)
                K = smo_ref.gram((call.X[idx] - mean) / scale, call.kernel, 1.0 / n_dims if gamma is None else gamma)
                alpha, _, _, _, _, status = svr_fit_ref.solve(K, call.y[idx], C, epsilon, call.eps, call.max_iter, trace)
                opposite = lambda s: (s["i"] < n) != (s["j"] < n)
            rows[call.family].add(len(idx))
            Cs.add(C)
            for step in trace:
                clips.update(step["branches"])
                tau = tau or step["tau"]
                if not step["branches"]:
                    unclipped.add("A" if opposite(step) else "B")
            rho.add("free" if np.any((alpha > 0) & (alpha < C)) else "bounds")
            stops.add(status)
    return Coverage(clips, unclipped, tau, rho, stops, rows, dims, kernels, Cs, per_call)


def check_coverage(c=None):
    c = coverage() if c is None else c
    assert c.clips == set(CLIPS), sorted(set(CLIPS) - c.clips)
    assert c.unclipped == {"A", "B"} and c.tau, (c.unclipped, c.tau)
    assert c.rho == {"free", "bounds"}, c.rho
    assert c.stops == {smo_ref.STATUS_CONVERGED, smo_ref.STATUS_NOT_CONVERGED}, c.stops
    assert c.rows["svr"] >= set(SVR_SIZE_ROWS) >= {1, 2, 31, 32, 33, 255, 256, 257, 300}, c.rows
    assert c.rows["svc"] >= set(SVC_SIZE_ROWS) >= {2, 31, 32, 33, 257}, c.rows
    assert max(max(v) for v in c.rows.values()) == 300
    assert c.dims >= {1, 8, 9, 34, 256}, c.dims
    assert c.kernels == {(f, k) for f in ("svc", "svr") for k in ("linear", "rbf")}, c.kernels
    assert c.Cs >= {C_SMALL, C_LARGE} and max(c.tasks_per_call) >= 9, (c.Cs, c.tasks_per_call)
    assert set(BUDGETS) == {1, 7, 0}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="assert the coverage of the calls on the CPU and stop")
    args = ap.parse_args()
    check_coverage()
    if args.check:
        print("coverage ok:", coverage())
        return
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import device_code_hash
    arrays = {}
    for call in calls():
        for suffix, kw in entry_points(call):
            first = None
            for budget in BUDGETS:                      # the record is one: the result does not depend on the budget
                got = run(call, budget, **kw)
                first = got if first is None else first
                assert all(np.array_equal(got[k], first[k]) for k in first), (call.name, suffix, budget)
            for key, value in first.items():
                arrays["%s%s.%s" % (call.name, suffix, key)] = value
    np.savez(args.out, kind=np.array("smo_bits"), compiler=np.array(device_code_hash.compiler_id() or ""), **arrays)
    print("%s: %d outputs, %d bytes" % (args.out, len(arrays), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
