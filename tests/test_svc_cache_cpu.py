"""CPU-side checks of the C-SVC solver's resident kernel matrices (DESIGN K23): the new symbols; the argument errors of the
*_cached entry points, which are reported before any device work; the layout (groups, first-appearance row lists, position lists,
chunks) of audioTrainTest.smo_cache_layout against hand-counted cases and of the library's own paa_debug_smo_cache_layout against
smo_cache_layout; the keyword validation of every Python entry point; and that the inputs of tests/test_svc_cache_gpu.py make the
sizes that file claims.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import svc_cache_cases as cases
from pyaudioanalysis_amd import _ffi, audioSegmentation as aS, audioTrainTest as aT
from test_platt_cpu import _Proba
from test_smo_cpu import _i32, _i64, _p, _Splits, _Tasks


def _f64(*v):
    return np.array(v, dtype=np.float64)


NEW_SYMBOLS = ("paa_smo_tasks_cached_f64", "paa_svc_fit_splits_cached_f64", "paa_svc_fit_proba_cached_f64", "paa_silence_batch_i16_cached",
               "paa_silence_batch_f64_cached", "paa_debug_smo_cache_layout")


class _TasksCached(_Tasks):
    """A valid two-task call of paa_smo_tasks_cached_f64 (the two tasks one group) whose arguments can be replaced one at a time."""

    def __init__(self):
        super().__init__()
        self.group, self.cache_bytes, self.cached = np.zeros(2, dtype=np.int32), 1 << 20, np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_smo_tasks_cached_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, self.n_tasks, _p(self.task_off, _ffi.c_i64p), _p(self.task_idx, _ffi.c_i32p),
            _p(self.task_sign, C.POINTER(C.c_int8)), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), _p(self.C, _ffi.c_f64p),
            _p(self.gamma, _ffi.c_f64p), self.kernel_type, self.eps, self.max_iter, self.ipl, _p(self.alpha_y, _ffi.c_f64p),
            _p(self.rho, _ffi.c_f64p), _p(self.iterations, _ffi.c_i32p), _p(self.gap, _ffi.c_f64p), _p(self.status, _ffi.c_i32p), None,
            _p(self.group, _ffi.c_i32p), self.cache_bytes, _p(self.cached, _ffi.c_i32p))


class _SplitsCached(_Splits):
    def __init__(self):
        super().__init__()
        self.cache_bytes, self.cached = 1 << 20, np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_svc_fit_splits_cached_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.labels, _ffi.c_i32p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.test_off, _ffi.c_i64p), _p(self.test_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p),
            _p(self.std, _ffi.c_f64p), _p(self.C, _ffi.c_f64p), _p(self.gamma, _ffi.c_f64p), self.kernel_type, self.eps, self.max_iter,
            self.ipl, _p(self.label_out, _ffi.c_i32p), _p(self.dec_out, _ffi.c_f64p), self.max_pairs, self.n_tasks,
            _p(self.task_iterations, _ffi.c_i32p), None, None, None, self.cache_bytes, _p(self.cached, _ffi.c_i32p))


class _ProbaCached(_Proba):
    def __init__(self):
        super().__init__()
        self.cache_bytes, self.cached = 1 << 20, np.zeros(1, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_svc_fit_proba_cached_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.labels, _ffi.c_i32p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), _p(self.C, _ffi.c_f64p),
            _p(self.gamma, _ffi.c_f64p), self.kernel_type, self.eps, self.max_iter, self.ipl, _p(self.seed, _ffi.c_i64p), self.n_pairs,
            self.n_rows, _p(self.alpha_y, _ffi.c_f64p), _p(self.rho, _ffi.c_f64p), _p(self.prob_a, _ffi.c_f64p), _p(self.prob_b, _ffi.c_f64p),
            _p(self.n_sv, _ffi.c_i32p), _p(self.task_it, _ffi.c_i32p), _p(self.task_status, _ffi.c_i32p), _p(self.sig_it, _ffi.c_i32p),
            _p(self.sig_stop, _ffi.c_i32p), None, None, self.cache_bytes, _p(self.cached, _ffi.c_i32p))


def test_new_symbols_are_declared_exported_and_in_the_header():
    import conftest
    from pyaudioanalysis_amd import _build
    header = open(os.path.join(conftest.ROOT, "include", "paa_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s) and re.search(r"^int %s\(" % s, header, re.M), s
    assert "kernels_smocache.hpp" in _build.HEADERS and "lib_gramcache.hpp" in _build.HEADERS and len(_build.SOURCES) == 18
    src = open(os.path.join(conftest.ROOT, "pyaudioanalysis_amd", "csrc", "family_smo.hip")).read()
    assert '#include "kernels_smocache.hpp"' in src
    # one packing rule and one Gram chain in the library
    csrc = os.path.join(conftest.ROOT, "pyaudioanalysis_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc)}
    assert [f for f, t in text.items() if "static int svr_cache_pack(" in t] == ["lib_gramcache.hpp"]
    assert [f for f, t in text.items() if "void svr_gram_kernel(" in t] == ["kernels_svrcache.hpp"]
    assert "__shared__" not in text["kernels_smocache.hpp"] and "extern __shared__" not in text["kernels_smocache.hpp"]


def test_cached_tasks_reject_bad_arguments_before_any_device_work():
    for name in ("X", "task_off", "task_idx", "task_sign", "mean", "std", "C", "gamma", "alpha_y", "rho", "iterations", "gap", "status", "cached"):
        assert _TasksCached()(**{name: None}) == _ffi.ERR_ARG, name
    for kw in (dict(cache_bytes=0), dict(cache_bytes=-1), dict(cache_bytes=-2**40)):
        assert _TasksCached()(**kw) == _ffi.ERR_ARG and "cache_bytes" in _ffi.last_error(), kw
    # the parent's arguments are judged first
    assert _TasksCached()(cache_bytes=0, eps=0.0) == _ffi.ERR_ARG and "eps" in _ffi.last_error()
    assert _TasksCached()(task_idx=_i32(0, 1, 2, 3, 6)) == _ffi.ERR_ARG
    assert _TasksCached()(n_dims=257) == _ffi.ERR_UNSUPPORTED
    # a group's tasks share every byte of mean, scale and gamma; the message names the two tasks
    other = np.zeros((2, 3))
    other[1, 2] = -0.0                                   # equal as a number, another byte
    for kw, what in ((dict(mean=other), "mean"), (dict(std=np.array([[1.0, 1, 1], [1, 1, 1 + 2.0**-52]])), "scale"),
                     (dict(gamma=_f64(0.5, 0.5 + 2.0**-53)), "gamma")):
        assert _TasksCached()(**kw) == _ffi.ERR_ARG, what
        assert "tasks 0 and 1" in _ffi.last_error() and what in _ffi.last_error(), _ffi.last_error()
        # ... also under the linear kernel, which reads no gamma; not when the tasks are their own groups
        assert _TasksCached()(kernel_type=0, **kw) == _ffi.ERR_ARG
        for group in (None, _i32(4, 5)):
            assert _TasksCached()(group=group, **kw) not in (_ffi.ERR_ARG, _ffi.ERR_UNSUPPORTED)
    if _ffi.device_count() < 1:                           # a valid call reaches the device and is refused there, never computed on the CPU
        assert _TasksCached()() not in (_ffi.PAA_OK, _ffi.ERR_ARG, _ffi.ERR_UNSUPPORTED)
        assert _TasksCached()(group=None) not in (_ffi.PAA_OK, _ffi.ERR_ARG, _ffi.ERR_UNSUPPORTED)


def test_cached_sweeps_reject_bad_arguments_before_any_device_work():
    for call, flags in ((_SplitsCached, "cached"), (_ProbaCached, "cached")):
        assert call()(**{flags: None}) == _ffi.ERR_ARG
        for kw in (dict(cache_bytes=0), dict(cache_bytes=-8)):
            assert call()(**kw) == _ffi.ERR_ARG and "cache_bytes" in _ffi.last_error(), kw
        assert call()(cache_bytes=0, max_iter=0) == _ffi.ERR_ARG and "max_iter" in _ffi.last_error()
        assert call()(n_dims=257) == _ffi.ERR_UNSUPPORTED
    assert _SplitsCached()(train_idx=_i32(0, 1, 2, 3, 4, 6)) == _ffi.ERR_ARG
    assert _ProbaCached()(seed=_i64(-1)) == _ffi.ERR_ARG
    # the silence batch: the budget is judged with the first arguments
    lib = _ffi.lib()
    z = np.zeros(8)
    i32, i64, u8 = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.uint8)
    f, p32, p64, pu = (lambda a: _p(a, _ffi.c_f64p)), (lambda a: _p(a, _ffi.c_i32p)), (lambda a: _p(a, _ffi.c_i64p)), (lambda a: _p(a, _ffi.c_u8p))
    outs = (pu(u8), pu(u8), pu(u8), f(z), f(z), f(z), p32(i32), f(z), f(z), p32(i32), f(z), f(z), f(z), f(z), f(z), p32(i32), p32(i32), p32(i32),
            p32(i32), p32(i32), None)
    head = (f(z), p64(_i64(0, 8)), 1, 16000.0, 4, 2, p32(i32), f(z), p64(i64), 0, p64(_i64(0, 8)))
    assert lib.paa_silence_batch_f64_cached(*head, *outs, 0, p32(i32)) == _ffi.ERR_ARG and "cache_bytes" in _ffi.last_error()
    assert lib.paa_silence_batch_f64_cached(*head, *outs, 1 << 20, None) == _ffi.ERR_ARG


def run_debug_layout(task_rows, groups, budget):
    rows = [np.asarray(r, dtype=np.int32) for r in task_rows]
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    idx = np.ascontiguousarray(np.concatenate(rows), dtype=np.int32)
    ids = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    n_groups = np.zeros(1, dtype=np.int32)
    group_of, chunk = np.zeros(n, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    group_off, group_rows, pos = np.zeros(n + 1, dtype=np.int64), np.zeros(len(idx), dtype=np.int32), np.zeros(len(idx), dtype=np.int32)
    rc = _ffi.lib().paa_debug_smo_cache_layout(n, _p(off, _ffi.c_i64p), _p(idx, _ffi.c_i32p), _p(ids, _ffi.c_i32p), int(budget),
                                               _p(n_groups, _ffi.c_i32p), _p(group_of, _ffi.c_i32p), _p(group_off, _ffi.c_i64p),
                                               _p(group_rows, _ffi.c_i32p), _p(pos, _ffi.c_i32p), _p(chunk, _ffi.c_i32p))
    assert rc == _ffi.PAA_OK, _ffi.last_error()
    g = int(n_groups[0])
    return (group_of.tolist(), [group_rows[group_off[k]:group_off[k + 1]].tolist() for k in range(g)],
            [pos[off[t]:off[t + 1]].tolist() for t in range(n)], chunk[:g].tolist())


def restated(task_rows, groups, budget):
    group_of, group_rows, pos, chunk = aT.smo_cache_layout(task_rows, groups, budget)
    return group_of.tolist(), [r.tolist() for r in group_rows], [p.tolist() for p in pos], chunk.tolist()


def test_layout_against_hand_counted_cases():
    for task_rows, groups, budget, group_of, group_rows, pos, chunk in cases.LAYOUTS_BY_HAND:
        want = (group_of, group_rows, pos, chunk)
        assert restated(task_rows, groups, budget) == want, (task_rows, groups, budget)
        assert run_debug_layout(task_rows, groups, budget) == want, (task_rows, groups, budget)


def test_the_librarys_layout_is_the_restatement_on_a_random_sweep():
    kinds = set()
    for seed in range(300):
        task_rows, groups, budget = cases.random_layout_case(seed)
        want = restated(task_rows, groups, budget)
        assert run_debug_layout(task_rows, groups, budget) == want, seed
        # what a layout is: every task row finds its sample at its place; a group's rows are distinct; chunks in group order
        for t, rows in enumerate(task_rows):
            g = want[0][t]
            assert [want[1][g][p] for p in want[2][t]] == list(rows)
        for rows in want[1]:
            assert len(set(rows)) == len(rows)
        kept = [c for c in want[3] if c >= 0]
        assert kept == sorted(kept) and (not kept or kept[0] == 0)
        kinds.add((len(kept) < len(want[3]), max(want[3], default=-1) > 0, groups is None))
    assert len(kinds) >= 6                                # cached and not, one chunk and several, with ids and without
    # and on the inputs of the GPU tests
    X, tasks, groups, names = cases.mixed_batch(9)
    rows = [t[0] for t in tasks]
    for budget in (1 << 30, cases.matrix_bytes(513), cases.matrix_bytes(513) - 1, 8):
        assert run_debug_layout(rows, groups, budget) == restated(rows, groups, budget)
    bad = np.zeros(3, dtype=np.int32)
    lib = _ffi.lib()
    args = lambda budget, idx: (1, _p(_i64(0, 3), _ffi.c_i64p), _p(idx, _ffi.c_i32p), None, budget, _p(bad, _ffi.c_i32p), _p(bad, _ffi.c_i32p),  # noqa: E731
                                _p(_i64(0, 0), _ffi.c_i64p), _p(bad, _ffi.c_i32p), _p(bad, _ffi.c_i32p), _p(bad, _ffi.c_i32p))
    assert lib.paa_debug_smo_cache_layout(*args(0, _i32(0, 1, 2))) == _ffi.ERR_ARG
    assert lib.paa_debug_smo_cache_layout(*args(64, _i32(0, -1, 2))) == _ffi.ERR_ARG


@pytest.mark.parametrize("n_dims", cases.DIMS)
def test_the_gpu_inputs_make_the_sizes_they_claim(n_dims):
    X, tasks, groups, names = cases.mixed_batch(n_dims)
    assert X.shape == (cases.N_SAMPLES, n_dims) and len(tasks) == len(groups) == len(names) == 6 + 3 + 6 + 1 + 4
    by = dict(zip(names, tasks))
    assert [len(by["size%d" % n][0]) for n in cases.SIZE_ROWS] == [1, 2, 255, 256, 257, 513]
    assert sorted(by["size2"][1].tolist()) == [-1.0, 1.0]
    for name, task in by.items():
        assert len(task[0]) == len(task[1]) and set(task[1].tolist()) <= {1.0, -1.0} and task[2].shape == task[3].shape == (n_dims,)
        assert np.all(task[3] > 0) and (len(task[0]) < 2 or len(set(task[1].tolist())) == 2), name
    group_of, group_rows, pos, chunk = aT.smo_cache_layout([t[0] for t in tasks], groups, 1 << 30)
    assert np.array_equal(group_of, groups) and chunk.tolist() == [0] * 11
    sizes = cases.group_sizes(tasks, groups)
    assert [len(r) for r in group_rows] == list(sizes.values()) == [1, 2, 255, 256, 257, 513, 210, 120, 8, 60, 60]
    # the pair tasks of three classes share rows: every class is in two tasks, and a task reads two runs of the group's row list
    three = [by["three_%s" % p] for p in ("01", "02", "12")]
    assert [len(t[0]) for t in three] == [160, 140, 120] and len(set(np.concatenate([t[0] for t in three]).tolist())) == 210
    p02 = pos[names.index("three_02")]
    assert p02.tolist() == list(range(90)) + list(range(160, 210))
    # the folds: permuted subsets of the pair, grouped by sign, with position lists that are not monotone
    pair = by["pair"]
    assert len(pair[0]) == 120
    for f in range(5):
        task, p = by["fold%d" % f], pos[names.index("fold%d" % f)]
        assert len(task[0]) == 96 and set(task[0].tolist()) < set(pair[0].tolist()) and np.any(np.diff(p) < 0)
        assert np.array_equal(pair[0][p], task[0]) and np.array_equal(pair[1][p], task[1])
        assert np.count_nonzero(np.diff(task[1]) != 0) == 1
        assert task[2].tobytes() == pair[2].tobytes() and task[3].tobytes() == pair[3].tobytes()
    # one sample twice: both rows at one place
    twice, p = by["twice"], pos[names.index("twice")]
    assert len(twice[0]) == 9 and twice[0][0] == twice[0][4] and p[0] == p[4] == 0 and len(set(p.tolist())) == 8
    # two gammas over the same rows and statistics
    assert by["gamma_a0"][5] != by["gamma_b0"][5] and by["gamma_a0"][0].tobytes() == by["gamma_b0"][0].tobytes()
    assert by["gamma_a1"][2].tobytes() == by["gamma_b1"][2].tobytes() and np.any(np.diff(pos[names.index("gamma_b1")]) < 0)


def test_the_big_groups_pass_4_gib_in_one_chunk():
    X, tasks, groups = cases.big_groups()
    rows = [t[0] for t in tasks]
    assert X.shape == (cases.MAX_ROWS + 500, 1) and len(tasks) == 18 and [len(r) for r in rows] == [8192, 4096] * 9
    group_of, group_rows, pos, chunk = aT.smo_cache_layout(rows, groups, 5 << 30)
    assert [len(r) for r in group_rows] == [8192] * 9 and chunk.tolist() == [0] * 9
    assert 8 * cases.matrix_bytes(8192) == 4 << 30                  # the ninth matrix begins at byte offset 4 GiB
    assert aT.smo_cache_layout(rows, groups, 4 << 30)[3].tolist() == [0] * 8 + [1]
    assert all(np.any(np.diff(pos[2 * k + 1]) < 0) and len(set(t[1].tolist())) == 2 for k, t in enumerate(tasks[1::2]))


def test_python_entry_points_validate_the_keywords():
    X = np.zeros((6, 3))
    task = (np.array([0, 1, 2]), np.array([1, -1, 1]), np.zeros(3), np.ones(3), 1.0, None)
    job = (np.array([0, 1, 2, 3]), np.array([4, 5]), np.zeros(3), np.ones(3), 1.0)
    labels = np.array([0, 1, 0, 1, 0, 1])
    bad = (dict(kernel_cache="lru"), dict(kernel_cache="gram", cache_bytes=0), dict(kernel_cache="gram", cache_bytes=-5))
    clip = np.zeros(16000, dtype=np.int16)
    feats = [np.zeros((4, 3)), np.ones((4, 3))]
    for kw in bad:
        for call in (lambda: aT.smo_solve(X, [task], **kw), lambda: aT.svm_split_fit_predict(X, labels, [job], **kw),
                     lambda: aT.svc_fit_proba(X, labels, [job[:1] + job[2:]], **kw), lambda: aT.train_svm_device(X, labels, 1.0, **kw),
                     lambda: aT.evaluate_classifier(feats, ["a", "b"], "svm", [1.0], 0, svm_fit="device", **kw),
                     lambda: aT.evaluate_classifier_full(feats, ["a", "b"], "svm", [1.0], 0, svm_fit="device", **kw),
                     lambda: aT.extract_features_and_train(["/nonexistent"], 1.0, 1.0, 0.05, 0.05, "svm", "m", final_fit="device", **kw),
                     lambda: aS.silence_removal(clip, 16000, 0.05, 0.05, svm_fit="device", **kw),
                     lambda: aS.silence_removal_batch([clip], 16000, 0.05, 0.05, **kw),
                     lambda: aS.silence_removal_files(["/nonexistent.wav"], 0.05, 0.05, **kw)):
            with pytest.raises(ValueError, match="kernel_cache|cache_bytes"):
                call()
    # read under the device modes only
    for kw in (dict(kernel_cache="gram"), dict(cache_bytes=1 << 20)):
        for call in (lambda: aT.evaluate_classifier(feats, ["a", "b"], "svm", [1.0], 0, **kw),
                     lambda: aT.evaluate_classifier_full(feats, ["a", "b"], "svm", [1.0], 0, svm_fit="sklearn", **kw),
                     lambda: aT.extract_features_and_train(["/nonexistent"], 1.0, 1.0, 0.05, 0.05, "svm", "m", **kw),
                     lambda: aS.silence_removal(clip, 16000, 0.05, 0.05, **kw)):
            with pytest.raises(ValueError, match="device"):
                call()
    # groups: one id per task, under "gram" alone
    with pytest.raises(ValueError, match="groups"):
        aT.smo_solve(X, [task], groups=[0])
    with pytest.raises(ValueError, match="group ids"):
        aT.smo_solve(X, [task], kernel_cache="gram", groups=[0, 1])
    with pytest.raises(ValueError, match="group ids"):
        aT.smo_cache_layout([[0, 1]], [0, 1], 64)
    for fn in (aT.smo_solve, aT.svm_split_fit_predict, aT.svc_fit_proba, aT.train_svm_device, aT.evaluate_classifier,
               aT.evaluate_classifier_full, aT.extract_features_and_train, aS.silence_removal, aS.silence_removal_batch,
               aS.silence_removal_files):
        params = inspect.signature(fn).parameters
        for name, default in (("kernel_cache", "none"), ("cache_bytes", None)):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, (fn.__name__, name)
    assert inspect.signature(aT.smo_solve).parameters["groups"].kind is inspect.Parameter.KEYWORD_ONLY
    # the result types keep their positional fields; the flags come last and default to "not cached"
    assert list(inspect.signature(aT.SmoResult.__init__).parameters)[1:] == ["alpha_y", "rho", "iterations", "gap", "status", "n_launches", "cached"]
    assert list(inspect.signature(aT.SvmSplitResult.__init__).parameters)[1:] == ["label", "decision", "test_off", "classes", "task_off", "iterations",
                                                                                 "status", "n_sv", "n_launches", "cached"]
    assert not aT.SmoResult([], np.zeros(2), None, None, None, 0).cached.any()
