"""diarize_features_batch without a device: the restated NumPy sums of the device seeding against NumPy itself, the up-front
draw schedule against a traced loop of the restatement's seeding, the chunk packer, the refusals (raised before the library is
loaded) and the place of the new symbols and kernels in the header, the binding and the build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diar_batch_cases as cases
import diar_np_sums
import diar_ref
from conftest import ROOT
from pyaudioanalysis_amd import _build, _ffi, audioSegmentation as aS

NEW_SYMBOLS = ("paa_diar_batch_prepare_f64", "paa_diar_batch_sweep_f64", "paa_diar_batch_gather_f64")
SUM_SIZES = (1, 7, 8, 9, 127, 128, 129, 257, 8191, 8192, 8193, 16385, 36000)


@pytest.fixture
def no_device(monkeypatch):
    """the library cannot be loaded: whatever reaches it fails the test"""
    def refuse():
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_ffi, "lib", refuse)


# ---- NumPy's sums -------------------------------------------------------------------------------------------------------------------
def _squares(n, seed):
    """squared distances as the seeding sums them: non-negative, spread over six decades, with exact zeros"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n) ** 2 * rng.choice([1e-3, 1.0, 1e3], n)
    a[rng.integers(n, size=max(n // 50, 1))] = 0.0
    return a


@pytest.mark.parametrize("n", SUM_SIZES)
def test_restated_sums_are_numpys(n):
    """closest.sum() on a fresh vector and on a row view of a 2-D array (closest = new[best]), new.sum(axis=1) on the
    [trials][n] array, and cumsum, each bit for bit"""
    closest = _squares(n, n)
    assert diar_np_sums.sum_1d(closest) == closest.sum()
    assert np.array_equal(diar_np_sums.cumsum(closest), np.cumsum(closest))
    for trials in (2, 3, 5):
        d2 = np.stack([_squares(n, 7 * n + j) for j in range(trials)])
        new = np.minimum(closest[None, :], d2)
        assert np.array_equal(diar_np_sums.sum_rows(new), new.sum(axis=1)), trials
        for j in range(trials):
            assert diar_np_sums.sum_1d(new[j]) == new[j].sum(), (trials, j)


def test_sums_are_chunked_not_pairwise_over_the_whole_vector():
    """the rule the restatement states: from 8193 elements on the whole-vector pairwise sum is another number (so a device sum
    that skipped the 8192-element chunks would be caught by the batch tests at those sizes)"""
    differ = 0
    for seed in range(8):
        a = _squares(8193 + 8 * seed, seed)
        differ += diar_np_sums.pairwise(a) != diar_np_sums.sum_1d(a)
        assert diar_np_sums.sum_1d(a) == a.sum()
    assert differ >= 1


# ---- the draw schedule --------------------------------------------------------------------------------------------------------------
def test_draws_up_front_equal_a_traced_loop():
    """one shared RandomState through the restatement's seeding of three clips (two sweeps and one fixed k, one k of clip 1 given)
    against the same seed drawn up front: the same calls with the same values in the same order"""
    plan = [(60, list(range(2, 10)), None), (45, list(range(2, 10)), {4: np.zeros((4, 5))}), (200, [17], None)]
    traced = cases.TracedRandomState(12)
    for n, ks, init in plan:
        Zk = np.random.default_rng(n).standard_normal((n, 5))
        for k in ks:
            if init is None or k not in init:
                diar_ref.seed_indices(Zk, k, traced)
    rs = np.random.RandomState(12)
    flat = []
    for n, ks, init in plan:
        draws, exc = aS._diar_batch_draws(rs, n, ks, init, 5)
        assert exc is None and [k for k, _, _ in draws] == ks
        for k, first, u in draws:
            if init is not None and k in init:
                assert first is None and u is None
                continue
            trials = 2 + int(np.log(k))
            assert u.shape == (k - 1, trials)
            flat.append(("randint", n, first))
            flat += [("uniform", trials, u[s]) for s in range(k - 1)]
    assert len(flat) == len(traced.trace)
    for got, want in zip(flat, traced.trace):
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]), (got, want)
    assert rs.randint(1 << 30) == traced.randint(1 << 30)            # and both states stand at the same place afterwards


def test_draws_stop_where_the_loop_raises():
    rs, ref = np.random.RandomState(3), np.random.RandomState(3)
    draws, exc = aS._diar_batch_draws(rs, 50, [2, 3, 4], {3: np.zeros((3, 7))}, 6)
    assert isinstance(exc, ValueError) and "init_centers[3] has shape (3, 7), (3, 6) expected" in str(exc)
    assert [k for k, _, _ in draws] == [2]
    aS._diar_batch_draws(ref, 50, [2], None, 6)
    assert rs.randint(1 << 30) == ref.randint(1 << 30)


def test_seed_draws_restatement_agrees():
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    want = diar_np_sums.seed_draws(a, 33, [2, 3, 9], given=(3,))
    draws, _ = aS._diar_batch_draws(b, 33, [2, 3, 9], {3: np.zeros((3, 4))}, 4)
    for k, first, u in draws:
        if k == 3:
            continue
        assert first == want[k][0] and np.array_equal(u, want[k][1])


# ---- the chunk packer ---------------------------------------------------------------------------------------------------------------
def test_chunks_keep_order_respect_the_bound_and_isolate_an_oversize_clip():
    n_dims = 20
    ns = [100, 5000, 120, 90, 130, 110]
    ks_list = [list(range(2, 10))] * 2 + [[3]] * 4
    need = [aS._diar_clip_bytes(n_dims, n, ks) for n, ks in zip(ns, ks_list)]
    assert need[1] > 4 * need[0]
    bound = need[2] + need[3] + need[4] // 2
    chunks = aS._diar_batch_chunks(n_dims, ns, ks_list, bound)
    assert [lo for lo, _ in chunks] == [0] + [hi for _, hi in chunks[:-1]] and chunks[-1][1] == len(ns)     # order, no gap
    for lo, hi in chunks:
        assert hi > lo and (hi - lo == 1 or sum(need[lo:hi]) <= bound)
    assert (1, 2) in chunks and need[1] > bound                    # the oversize clip runs alone
    assert (2, 4) in chunks
    assert aS._diar_batch_chunks(n_dims, ns, ks_list) == [(0, 6)]  # 1 GiB holds them all
    assert aS._diar_batch_chunks(n_dims, ns, ks_list, 1) == [(i, i + 1) for i in range(6)]
    assert aS._diar_batch_chunks(n_dims, [], [], 1) == []


def test_chunks_bound_the_jobs_of_a_launch():
    ns, ks_list = [40] * 3000, [list(range(2, 10))] * 3000
    chunks = aS._diar_batch_chunks(4, ns, ks_list, 1 << 40)
    assert len(chunks) == 3 and all(8 * (hi - lo) <= aS._DIAR_BATCH_MAX_JOBS for lo, hi in chunks)


def test_clip_bytes_cover_the_scratch_the_issue_names():
    """labels and d2 take jobs x n, the pair partials tiles x bins x 8: about 91 MB for a one-hour clip in the sweep"""
    n, ks = 36000, list(range(2, 10))
    tiles = (n // 128 + 1) * (n // 128 + 2) // 2
    assert aS._diar_clip_bytes(148, n, ks) >= 12 * len(ks) * n + 8 * tiles * sum(k * k for k in ks) > 90e6


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_clip_and_come_before_the_device(no_device):
    good = cases.planted(1, 40, 9, 3)
    with pytest.raises(ValueError, match="clip 1: 12 feature dims, clip 0 has 9"):
        aS.diarize_features_batch([good, cases.planted(2, 40, 12, 3)], 3)
    with pytest.raises(ValueError, match="clip 0: feature matrix of 257 dims x 40 windows: 1..256 dims"):
        aS.diarize_features_batch([np.zeros((257, 40))], 3)
    with pytest.raises(ValueError, match="clip 2: 8 windows are fewer than 9 clusters"):
        aS.diarize_features_batch([good, good, good[:, :8]], 0)
    with pytest.raises(ValueError, match="clip 1: 5 windows are fewer than 6 clusters"):
        aS.diarize_features_batch([good, good[:, :5]], [3, 6])
    with pytest.raises(ValueError, match="clip 1: 33 speakers: 1..32 clusters"):
        aS.diarize_features_batch([good, good], [3, 33])
    with pytest.raises(ValueError, match=r"clip 1: init_centers\[3\] has shape \(2, 4\)"):
        aS.diarize_features_batch([good, good], 3, init_centers=[None, {3: np.zeros((2, 4))}])
    with pytest.raises(ValueError, match=r"clip 0: init_centers\[3\] has shape \(3, 10\)"):
        aS.diarize_features_batch([good], 3, init_centers=[{3: np.zeros((3, 10))}])
    with pytest.raises(ValueError, match="clip 1: M must be"):
        aS.diarize_features_batch([good, np.zeros(5)], 3)
    with pytest.raises(ValueError, match="one int per clip"):
        aS.diarize_features_batch([good, good], [3])
    with pytest.raises(ValueError, match="one dict"):
        aS.diarize_features_batch([good, good], 3, init_centers=[None])
    with pytest.raises(ValueError, match="on_error"):
        aS.diarize_features_batch([good], 3, on_error="ignore")
    assert aS.diarize_features_batch([], 3) == []
    with pytest.raises(NotImplementedError, match="LDA"):
        aS.speaker_diarization_batch([np.zeros(16000)], 16000, 2, lda_dim=5)
    with pytest.raises(NotImplementedError, match="LDA"):
        aS.speaker_diarization_files(["nothing.wav"], 2, lda_dim=5)
    assert aS.speaker_diarization_batch([], 16000, 2, models=()) == []


def test_c_abi_refusals():
    """returned before the device is touched: on a host without a GPU anything later would be a HIP error"""
    lib = _ffi.lib()
    i64 = lambda v: _ffi.as_i64p(np.ascontiguousarray(v, dtype=np.int64))
    buf = np.zeros(64)
    P = buf.ctypes.data_as(C.c_void_p)
    Q = C.c_void_p(buf.ctypes.data + 8)

    def refused(rc, *needles):
        assert rc == _ffi.ERR_ARG, (rc, _ffi.last_error())
        for s in needles:
            assert s in _ffi.last_error(), _ffi.last_error()

    F = _ffi.as_f64p(np.zeros(4096))
    refused(lib.paa_diar_batch_prepare_f64(P, 0, 10, i64([0]), i64([10]), 1, Q, F, F), "feature dimensions")
    refused(lib.paa_diar_batch_prepare_f64(P, 257, 10, i64([0]), i64([10]), 1, Q, F, F), "feature dimensions")
    refused(lib.paa_diar_batch_prepare_f64(P, 4, 10, i64([0]), i64([10]), 0, Q, F, F), "clips")
    refused(lib.paa_diar_batch_prepare_f64(P, 4, 10, i64([0, 6]), i64([6, 5]), 2, Q, F, F), "clip 1")
    refused(lib.paa_diar_batch_prepare_f64(P, 4, 10, i64([0]), i64([0]), 1, Q, F, F), "clip 0")
    refused(lib.paa_diar_batch_prepare_f64(None, 4, 10, i64([0]), i64([10]), 1, Q, F, F), "null")
    refused(lib.paa_diar_batch_prepare_f64(P, 4, 10, i64([0]), i64([10]), 1, P, F, F), "buffer of its own")
    refused(lib.paa_diar_batch_gather_f64(P, 4, i64([-1]), i64([0]), i64([10]), 1, Q, 10), "slab offset")
    refused(lib.paa_diar_batch_gather_f64(P, 4, i64([0]), i64([5]), i64([10]), 1, Q, 10), "clip 0")

    def sweep(dims=(3,), rows=(0, 1, 2), nks=(1,), ks=(2,), tols=(1e-4,), max_iter=300, seeded=(1,), first=(0,), u=(0.5, 0.5),
              centers=None, ns=(10,)):
        i32 = lambda v: _ffi.as_i32p(np.ascontiguousarray(v, dtype=np.int32))
        cen = np.zeros(64) if centers is None else np.ascontiguousarray(centers, dtype=np.float64)
        out_i, out_f = np.zeros(8, dtype=np.int32), np.zeros(8 * 32 * 32)
        return lib.paa_diar_batch_sweep_f64(P, 4, 10, 1, i64([0]), i64(ns), i32(dims), i32(rows), i32(nks), i32(ks),
                                            _ffi.as_f64p(np.ascontiguousarray(tols, dtype=np.float64)), max_iter, i32(seeded), i64(first),
                                            _ffi.as_f64p(np.ascontiguousarray(u, dtype=np.float64)), _ffi.as_f64p(cen), Q,
                                            _ffi.as_i32p(out_i), _ffi.as_f64p(out_f), _ffi.as_f64p(out_f), _ffi.as_f64p(out_f), None)

    refused(sweep(dims=(5,)), "kept rows")
    refused(sweep(rows=(0, 1, 4)), "row 4")
    refused(sweep(nks=(0,)), "cluster counts")
    refused(sweep(ks=(33,)), "33 clusters")
    refused(sweep(ks=(11,), u=np.full(40, 0.5)), "11 clusters for 10 vectors")
    refused(sweep(tols=(-1.0,)), "tol")
    refused(sweep(max_iter=0), "max_iter")
    refused(sweep(first=(10,)), "first window")
    refused(sweep(u=(0.5, 1.0)), "seeding draw")
    refused(sweep(seeded=(0,), centers=np.full(64, np.nan)), "not finite")


# ---- ABI and build ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    handle = C.CDLL(_build.build())
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _ffi.EXPORTED_SYMBOLS
        assert hasattr(handle, name), name
    assert len(_ffi._SIGNATURES["paa_diar_batch_sweep_f64"][1]) == 22


def test_the_kernels_live_in_the_diarization_unit():
    assert "kernels_diarbatch.hpp" in _build.HEADERS and "lib_diar_batch.hpp" in _build.HEADERS
    unit = open(os.path.join(_build.CSRC, "family_diar.hip")).read()
    assert unit.index('#include "kernels_diar.hpp"') < unit.index('#include "kernels_diarbatch.hpp"')
    lib_unit = open(os.path.join(_build.CSRC, "paa_lib.hip")).read()
    assert lib_unit.index('#include "lib_diar.hpp"') < lib_unit.index('#include "lib_diar_batch.hpp"')
    kernels = open(os.path.join(_build.CSRC, "kernels_diarbatch.hpp")).read()
    for name in ("standardize_kernel", "dimdist_kernel", "dimdist_reduce_kernel", "seed_kernel", "assign_kernel", "update_kernel",
                 "finish_kernel", "row_sum_kernel", "pair_kernel", "pair_reduce_kernel"):
        assert re.search(r"void %s\(" % name, kernels), name
    body = re.sub(r"//[^\n]*", "", kernels)
    assert not re.search(r"atomicAdd\(\s*&?\s*\(?\s*double|atomicAdd\([^;]*(sums|d2|centers)\b", body)    # integer counters only
