"""music_thumbnailing_batch without a device: the ABI of the new entry points, every refusal of the C ABI (returned before the
device is touched: on a host without a GPU anything later would be PAA_ERR_HIP), the Python argument errors (raised before the
library is loaded), the place of the new kernels in the build, and the host-built tile / block lists of
csrc/lib_similarity_batch.hpp against a NumPy restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pyaudioanalysis_amd import _build, _ffi, audioSegmentation as aS

NEW_SYMBOLS = ("paa_dev_self_similarity_batch", "paa_dev_thumbnail_filter_batch", "paa_self_similarity_batch_f64",
               "paa_thumbnail_filter_batch_f64", "paa_thumbnail_batch_f64", "paa_music_thumbnail_batch_i16",
               "paa_music_thumbnail_batch_f64", "paa_music_thumbnail_batch_ptrs_i16", "paa_music_thumbnail_batch_ptrs_f64",
               "paa_debug_thumbnail_batch_layout")
MAX_VEC = 46340 * 4                 # paa_dev_self_similarity's bound


@pytest.fixture
def no_device(monkeypatch):
    """the library cannot be loaded: whatever reaches it fails the test"""
    def refuse():
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_ffi, "lib", refuse)


def i64(values):
    return np.ascontiguousarray(values, dtype=np.int64)


# ---- ABI and build ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    handle = C.CDLL(_build.build())
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _ffi.EXPORTED_SYMBOLS
        assert hasattr(handle, name), name
    i16, f64 = _ffi._SIGNATURES["paa_music_thumbnail_batch_i16"][1], _ffi._SIGNATURES["paa_music_thumbnail_batch_f64"][1]
    assert i16[0] is _ffi.c_i16p and f64[0] is _ffi.c_f64p and i16[1:] == f64[1:] and len(i16) == 14


def test_the_kernels_live_in_the_library_unit():
    assert len(_build.SOURCES) == 18 and "kernels_simbatch.hpp" in _build.HEADERS and "lib_similarity_batch.hpp" in _build.HEADERS
    unit = open(os.path.join(_build.CSRC, "paa_lib.hip")).read()
    assert unit.index('#include "kernels_sim.hpp"') < unit.index('#include "kernels_simbatch.hpp"')
    assert '#include "lib_similarity_batch.hpp"' in unit
    kernels = open(os.path.join(_build.CSRC, "kernels_simbatch.hpp")).read()
    for name in ("sim_row_stats_batch_kernel", "sim_normalize_batch_kernel", "sim_gram_batch_kernel", "thumb_diag_batch_kernel",
                 "thumb_min_batch_kernel", "thumb_fill_batch_kernel", "thumb_argmax_batch_kernel", "thumb_grow_batch_kernel"):
        assert "void %s(" % name in kernels
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in kernels and "atomic" not in kernels


# ---- refusals of the C ABI ----------------------------------------------------------------------------------------------------------
def _thumb_tail(n, m=4, band=2.0, l1=0.0, l2=1.0, pos=True, bounds=True):
    p, b = np.zeros((n, 2), dtype=np.int64), np.zeros((n, 4), dtype=np.int64)
    return (m, band, l1, l2, 0, _ffi.as_i64p(p) if pos else None, _ffi.as_i64p(b) if bounds else None, None), (p, b)


def _refused(rc, code, *needles):
    assert rc == code, (rc, _ffi.last_error())
    for s in needles:
        assert s in _ffi.last_error(), _ffi.last_error()


def test_self_similarity_batch_refusals():
    lib = _ffi.lib()
    feats, sim = np.zeros(5 * 30), np.zeros(3 * 100)
    nv = i64([10, 10, 10])
    F, S, N = _ffi.as_f64p(feats), _ffi.as_f64p(sim), _ffi.as_i64p(nv)
    _refused(lib.paa_self_similarity_batch_f64(None, 5, 3, N, 0, S), _ffi.ERR_ARG, "null")
    _refused(lib.paa_self_similarity_batch_f64(F, 5, 3, None, 0, S), _ffi.ERR_ARG, "null")
    _refused(lib.paa_self_similarity_batch_f64(F, 5, 3, N, 0, None), _ffi.ERR_ARG, "null")
    _refused(lib.paa_self_similarity_batch_f64(F, 5, 0, N, 0, S), _ffi.ERR_ARG, "0 clips")
    _refused(lib.paa_self_similarity_batch_f64(F, 0, 3, N, 0, S), _ffi.ERR_ARG, "0 rows")
    _refused(lib.paa_self_similarity_batch_f64(F, 5, 3, _ffi.as_i64p(i64([10, 0, 10])), 0, S), _ffi.ERR_ARG, "clip 1")
    _refused(lib.paa_self_similarity_batch_f64(F, 5, 3, _ffi.as_i64p(i64([10, 10, MAX_VEC + 1])), 0, S), _ffi.ERR_UNSUPPORTED, "clip 2")


@pytest.mark.parametrize("entry", ["features", "matrices"])
def test_thumbnail_batch_refusals(entry):
    lib = _ffi.lib()
    data = np.zeros(3 * 100)
    D = _ffi.as_f64p(data)

    def call(n_vec, n_clips=3, n_dims=5, data_p=D, **kw):
        tail, _ = _thumb_tail(3, **kw)
        N = None if n_vec is None else _ffi.as_i64p(i64(n_vec))
        if entry == "features":
            return lib.paa_thumbnail_batch_f64(data_p, n_dims, n_clips, N, *tail)
        return lib.paa_thumbnail_filter_batch_f64(data_p, n_clips, N, *tail)
    ok = [10, 10, 10]
    _refused(call(ok, data_p=None), _ffi.ERR_ARG, "null")
    _refused(call(None), _ffi.ERR_ARG, "null")
    _refused(call(ok, pos=False), _ffi.ERR_ARG, "null")
    _refused(call(ok, bounds=False), _ffi.ERR_ARG, "null")
    _refused(call(ok, n_clips=0), _ffi.ERR_ARG, "0 clips")
    _refused(call(ok, n_clips=-2), _ffi.ERR_ARG, "-2 clips")
    if entry == "features":
        _refused(call(ok, n_dims=0), _ffi.ERR_ARG, "0 rows")
    _refused(call([10, 3, 10]), _ffi.ERR_ARG, "clip 1", "fewer feature vectors (3)")
    _refused(call([10, 10, 3]), _ffi.ERR_ARG, "clip 2")
    _refused(call(ok, m=0), _ffi.ERR_ARG, "filter length 0")
    for bad in (-0.1, float("nan")):
        _refused(call(ok, l1=bad), _ffi.ERR_ARG, "limit_1 / limit_2")
        _refused(call(ok, l2=bad), _ffi.ERR_ARG, "limit_1 / limit_2")
    _refused(call([10, MAX_VEC + 1, 10]), _ffi.ERR_UNSUPPORTED, "clip 1", "too large")


@pytest.mark.parametrize("kind", ["i16", "f64"])
def test_music_thumbnail_batch_refusals(kind):
    lib = _ffi.lib()
    x = np.zeros(3000, dtype=np.int16 if kind == "i16" else np.float64)
    X = _ffi.as_i16p(x) if kind == "i16" else _ffi.as_f64p(x)
    fn = lib.paa_music_thumbnail_batch_i16 if kind == "i16" else lib.paa_music_thumbnail_batch_f64

    def call(offsets, n_clips=3, window=100, step=50, data_p=X, **kw):            # 1000 samples: 19 vectors
        tail, _ = _thumb_tail(3, **kw)
        return fn(data_p, None if offsets is None else _ffi.as_i64p(i64(offsets)), n_clips, 8000.0, window, step, *tail)
    ok = [0, 1000, 2000, 3000]
    _refused(call(ok, data_p=None), _ffi.ERR_ARG, "null")
    _refused(call(None), _ffi.ERR_ARG, "null")
    _refused(call(ok, pos=False), _ffi.ERR_ARG, "null")
    _refused(call(ok, bounds=False), _ffi.ERR_ARG, "null")
    _refused(call(ok, n_clips=0), _ffi.ERR_ARG, "0 clips")
    _refused(call(ok, window=1), _ffi.ERR_ARG, "window")
    _refused(call([0, 1000, 900, 3000]), _ffi.ERR_ARG, "clip 1", "do not ascend")
    _refused(call([0, 1000, 1099, 3000]), _ffi.ERR_ARG, "clip 1", "at least one array")          # 99 samples: no window
    _refused(call([0, 1000, 1200, 3000]), _ffi.ERR_ARG, "clip 1", "fewer feature vectors (3)")   # 200 samples: 3 vectors < 4
    _refused(call(ok, m=20), _ffi.ERR_ARG, "clip 0", "fewer feature vectors (19)")
    for bad in (-1.0, float("nan")):
        _refused(call(ok, l1=bad), _ffi.ERR_ARG, "limit_1 / limit_2")
        _refused(call(ok, l2=bad), _ffi.ERR_ARG, "limit_1 / limit_2")
    # a clip past the size bound: only its offsets say so (window 2, step 1: one vector per sample after the first)
    _refused(call([0, 1000, 1000 + MAX_VEC + 2, 1000 + MAX_VEC + 1002], window=2, step=1), _ffi.ERR_UNSUPPORTED, "clip 1", "too large")
    # the form with one pointer per clip refuses the same, and a clip without a buffer
    fn = lib.paa_music_thumbnail_batch_ptrs_i16 if kind == "i16" else lib.paa_music_thumbnail_batch_ptrs_f64
    ptrs = (C.c_void_p * 3)(x.ctypes.data, x.ctypes.data, x.ctypes.data)
    _refused(call(ok, data_p=None), _ffi.ERR_ARG, "null")
    _refused(call(ok, data_p=(C.c_void_p * 3)(x.ctypes.data, None, x.ctypes.data)), _ffi.ERR_ARG, "clip 1: null buffer")
    _refused(call([0, 1000, 1200, 3000], data_p=ptrs), _ffi.ERR_ARG, "clip 1", "fewer feature vectors (3)")
    _refused(call(ok, data_p=ptrs, l2=float("nan")), _ffi.ERR_ARG, "limit_1 / limit_2")


def test_device_buffer_entry_points_refuse_before_the_device():
    """the refusing calls never read what the pointers name: any non-null value stands for a device buffer"""
    lib = _ffi.lib()
    buf = np.zeros(64)
    P = C.c_void_p(buf.ctypes.data)
    z3, nv = _ffi.as_i64p(i64([0, 0, 0])), _ffi.as_i64p(i64([10, 10, 10]))
    sim = lib.paa_dev_self_similarity_batch
    _refused(sim(None, 5, 3, z3, nv, nv, P, z3), _ffi.ERR_ARG, "null")
    _refused(sim(P, 5, 3, z3, nv, nv, None, z3), _ffi.ERR_ARG, "null")
    _refused(sim(P, 5, 3, None, nv, nv, P, z3), _ffi.ERR_ARG, "null")
    _refused(sim(P, 5, 0, z3, nv, nv, P, z3), _ffi.ERR_ARG, "0 clips")
    _refused(sim(P, 0, 3, z3, nv, nv, P, z3), _ffi.ERR_ARG, "0 rows")
    _refused(sim(P, 5, 3, z3, nv, _ffi.as_i64p(i64([10, 9, 10])), P, z3), _ffi.ERR_ARG, "clip 1", "ld 9")
    _refused(sim(P, 5, 3, _ffi.as_i64p(i64([0, 0, -8])), nv, nv, P, z3), _ffi.ERR_ARG, "clip 2")
    _refused(sim(P, 5, 3, z3, _ffi.as_i64p(i64([MAX_VEC + 1, 10, 10])), nv, P, z3), _ffi.ERR_UNSUPPORTED, "clip 0")
    filt = lib.paa_dev_thumbnail_filter_batch
    _refused(filt(None, z3, nv, 3, 4, 2.0, 0.0, 1.0, P, z3, P, P), _ffi.ERR_ARG, "null")
    _refused(filt(P, z3, nv, 3, 4, 2.0, 0.0, 1.0, P, z3, None, P), _ffi.ERR_ARG, "null")
    _refused(filt(P, z3, nv, 3, 4, 2.0, 0.0, 1.0, P, z3, P, None), _ffi.ERR_ARG, "null")
    _refused(filt(P, z3, nv, 0, 4, 2.0, 0.0, 1.0, P, z3, P, P), _ffi.ERR_ARG, "0 clips")
    _refused(filt(P, z3, nv, 3, 11, 2.0, 0.0, 1.0, P, z3, P, P), _ffi.ERR_ARG, "clip 0", "fewer feature vectors (10)")
    _refused(filt(P, z3, nv, 3, 4, 2.0, float("nan"), 1.0, P, z3, P, P), _ffi.ERR_ARG, "limit_1 / limit_2")
    _refused(filt(P, z3, nv, 3, 4, 2.0, 0.0, -1.0, P, z3, P, P), _ffi.ERR_ARG, "limit_1 / limit_2")
    _refused(filt(P, z3, _ffi.as_i64p(i64([10, 10, MAX_VEC + 1])), 3, 4, 2.0, 0.0, 1.0, P, z3, P, P), _ffi.ERR_UNSUPPORTED, "clip 2")


# ---- Python argument errors ---------------------------------------------------------------------------------------------------------
def test_an_empty_list_returns_an_empty_list(no_device):
    assert aS.music_thumbnailing_batch([], 8000) == []
    assert aS.music_thumbnailing_files([]) == []
    assert aS.self_similarity_batch([]) == [] and aS.thumbnail_batch([], 4, 2.0) == [] and aS.thumbnail_filter_batch([], 4, 2.0) == []


def test_a_clip_shorter_than_one_window_is_refused_before_the_device(no_device):
    ok, short = np.zeros(12 * 8000, dtype=np.int16), np.zeros(7999, dtype=np.int16)
    with pytest.raises(ValueError, match=r"clip 1: need at least one array to concatenate"):
        aS.music_thumbnailing_batch([ok, short, ok], 8000)
    with pytest.raises(ValueError, match=r"clip 2: need at least one array to concatenate"):
        aS.music_thumbnailing_batch([ok, np.double(ok), np.stack([short, short], axis=1)], 8000)


def test_a_clip_with_fewer_vectors_than_the_filter_is_refused_before_the_device(no_device):
    ok, few = np.zeros(12 * 8000, dtype=np.int16), np.zeros(10 * 8000, dtype=np.int16)      # 23 and 19 vectors, a filter of 20
    with pytest.raises(ValueError, match=r"clip 2: 19 feature vectors are fewer than the thumbnail filter length 20"):
        aS.music_thumbnailing_batch([ok, ok, few], 8000)
    window, step, m_filter, frames = aS._thumb_plan([12 * 8000, 10 * 8000], 8000, 1.0, 0.5, 9.0)
    assert (window, step, m_filter, frames.tolist()) == (8000, 4000, 18, [23, 19])
    with pytest.raises(ValueError, match=r"clip 0: 2 feature vectors are fewer"):
        aS.thumbnail_batch([np.zeros((5, 2)), np.zeros((5, 9))], 3, 1.0)
    with pytest.raises(ValueError, match=r"clip 1: 2 feature vectors are fewer"):
        aS.thumbnail_filter_batch([np.eye(9), np.eye(2)], 3, 1.0)
    with pytest.raises(ValueError, match=r"clip 1: 4 feature rows, clip 0 has 5"):
        aS.self_similarity_batch([np.zeros((5, 9)), np.zeros((4, 9))])
    with pytest.raises(ValueError, match=r"clip 1: feature_vectors must be a non-empty"):
        aS.self_similarity_batch([np.zeros((5, 9)), np.zeros((5, 0))])
    with pytest.raises(ValueError, match=r"clip 0: a similarity matrix is square"):
        aS.thumbnail_filter_batch([np.zeros((3, 4))], 2, 1.0)


def test_files_are_checked_before_the_device(no_device, tmp_path):
    import scipy.io.wavfile as wavfile
    paths = [str(tmp_path / n) for n in ("ok.wav", "ok_16k.wav", "few.wav", "short.wav")]
    wavfile.write(paths[0], 8000, np.zeros(12 * 8000, dtype=np.int16))
    wavfile.write(paths[1], 16000, np.zeros(12 * 16000, dtype=np.int16))
    wavfile.write(paths[2], 8000, np.zeros(10 * 8000, dtype=np.int16))
    wavfile.write(paths[3], 16000, np.zeros(15999, dtype=np.int16))
    with pytest.raises(ValueError, match=r"clip 2: 19 feature vectors are fewer"):          # named by its place among the paths
        aS.music_thumbnailing_files(paths[:3])
    with pytest.raises(ValueError, match=r"clip 3: need at least one array"):
        aS.music_thumbnailing_files(paths[:2] + [paths[0], paths[3]])
    with pytest.raises(ValueError, match=r"file 1 .*cannot be read"):
        aS.music_thumbnailing_files([paths[0], str(tmp_path / "missing.wav")])


def test_sample_types_travel_as_two_groups(monkeypatch):
    """int16 clips as int16, every other clip through np.double: each clip takes the sample path of its own single call"""
    calls = []

    def capture(clips, as_i16, fs, window, step, frames, m_filter, band, l1, l2, want, chunk_bytes):
        calls.append((as_i16, [c.dtype for c in clips], [c.shape[0] for c in clips], frames.tolist(), m_filter, band))
        return [((0, 0), (0, 0, 0, 0), None)] * len(clips)
    monkeypatch.setattr(aS, "_thumb_group", capture)
    a, b = np.zeros(12 * 8000, dtype=np.int16), np.zeros(13 * 8000, dtype=np.int16)
    out = aS.music_thumbnailing_batch([a, np.float32(b), np.stack([a, a], axis=1), b], 8000, return_details=True)
    assert calls == [(True, [np.dtype(np.int16)] * 2, [96000, 104000], [23, 25], 20, 10.0),
                     (False, [np.dtype(np.float64)] * 2, [104000, 96000], [25, 23], 20, 10.0)]
    assert out == [(0.0, 0.0, 0.0, 0.0, (0, 0))] * 4


# ---- host-built lists ----------------------------------------------------------------------------------------------------------------
def _layout(n_vec, n_dims, m):
    n_vec = i64(n_vec)
    n = len(n_vec)
    counts = np.zeros(3, dtype=np.int64)
    cap = 1 << 16
    tiles, blocks, rows = (np.full((cap, 3), -1, dtype=np.int32) for _ in range(3))
    clip_off = np.zeros((n, 3), dtype=np.int64)
    _ffi.check(_ffi.lib().paa_debug_thumbnail_batch_layout(_ffi.as_i64p(n_vec), n, n_dims, m, _ffi.as_i64p(counts), _ffi.as_i32p(tiles), cap,
                                                           _ffi.as_i32p(blocks), cap, _ffi.as_i32p(rows), cap, _ffi.as_i64p(clip_off)))
    return tiles[:counts[0]], blocks[:counts[1]], rows[:counts[2]], clip_off


def _restated(n_vec, n_dims, m):
    tiles, blocks, rows, offs = [], [], [], []
    z = aux = cand = 0
    dims_pad = -(-n_dims // 4) * 4
    for c, T in enumerate(n_vec):
        nt, R = -(-T // 128), T - m + 1
        gx, gy = -(-R // 256), -(-R // 32)
        offs.append((z, aux, cand))
        z, aux, cand = z + dims_pad * nt * 128, aux + 2 * n_dims + nt * 128, cand + 3 * gx * gy + 2
        tiles += [(c, ti, tj) for ti in range(nt) for tj in range(ti, nt)]
        # a block holds a cell when its first diagonal offset 256 bx, at its first row 32 by, lies inside the R x R matrix
        blocks += [(c, bx, by) for by in range(gy) for bx in range(gx) if 32 * by + 256 * bx < R]
        rows += [(c, 0, by) for by in range(-(-R // 8))]
    return tiles, blocks, rows, offs


@pytest.mark.parametrize("n_vec,n_dims,m", [((1, 2, 127, 128, 129, 257, 385), 68, 1), ((385, 257, 129, 128, 127, 2, 1), 5, 1),
                                             ((32, 33, 63, 64, 65, 287), 68, 32), ((300, 600, 1100, 20), 34, 20),
                                             ((2079,), 3, 31)])
def test_host_built_lists_match_the_restatement(n_vec, n_dims, m):
    tiles, blocks, rows, clip_off = _layout(n_vec, n_dims, m)
    want_tiles, want_blocks, want_rows, want_off = _restated(n_vec, n_dims, m)
    assert [tuple(t) for t in tiles.tolist()] == want_tiles                  # clip-major, every (clip, ti <= tj) once
    assert len(set(want_tiles)) == len(want_tiles) and all(ti <= tj for _, ti, tj in want_tiles)
    assert sorted(tuple(b) for b in blocks.tolist()) == sorted(want_blocks) and len(set(want_blocks)) == len(want_blocks)
    assert [tuple(r) for r in rows.tolist()] == want_rows
    assert clip_off.tolist() == [list(o) for o in want_off]
    for c, bx, by in blocks.tolist():                                         # no block without a cell, no cell without a block
        R = n_vec[c] - m + 1
        assert R - 32 * by - 256 * bx > 0
    for c, T in enumerate(n_vec):
        R = T - m + 1
        mine = {by * 4096 + bx for cc, bx, by in blocks.tolist() if cc == c}
        i, j = np.triu_indices(R)
        assert set(np.unique((i // 32) * 4096 + (j - i) // 256).tolist()) == mine


def test_offsets_are_64_bit():
    """300 clips of 65535 feature rows: Z of a clip is 65536 x 128 doubles, so the offsets pass 2^31 doubles"""
    n_vec = [100] * 300
    tiles, blocks, rows, clip_off = _layout(n_vec, 65535, 10)
    assert len(tiles) == 300 and len(blocks) == 300 * 3 and clip_off.dtype == np.int64
    assert clip_off[:, 0].tolist() == [c * 65536 * 128 for c in range(300)] and clip_off[-1, 0] > 2 ** 31
    assert clip_off[:, 1].tolist() == [c * (2 * 65535 + 128) for c in range(300)]


def test_layout_refuses_what_the_batch_refuses():
    lib = _ffi.lib()
    counts, lists, off = np.zeros(3, dtype=np.int64), np.zeros((4, 3), dtype=np.int32), np.zeros((2, 3), dtype=np.int64)
    L, nv = _ffi.as_i32p(lists), _ffi.as_i64p(i64([300, 5]))
    _refused(lib.paa_debug_thumbnail_batch_layout(nv, 2, 68, 6, _ffi.as_i64p(counts), L, 4, L, 4, L, 4, _ffi.as_i64p(off)), _ffi.ERR_ARG, "clip 1")
    _refused(lib.paa_debug_thumbnail_batch_layout(nv, 2, 68, 5, _ffi.as_i64p(counts), L, 4, L, 4, L, 4, _ffi.as_i64p(off)), _ffi.ERR_ARG, "do not fit")
    assert counts.tolist() == [6 + 1, 10 + 2 + 1, 37 + 1]          # 3 x 3 tiles above the diagonal; R = 296: 10 rows of blocks, two of them reach bx = 1


# ---- constructed inputs of the GPU tests ---------------------------------------------------------------------------------------------
def test_grow_cases_hit_the_break_conditions_they_are_named_for():
    import sim_ref
    import thumb_batch_cases as cases
    seen = set()
    for name, (S, want_pos, (stop, back, fwd, ties)) in cases.grow_cases().items():
        assert np.array_equal(np.nan_to_num(S, nan=7.0), np.nan_to_num(S.T, nan=7.0)), name
        filtered = np.asarray(sim_ref.thumbnail_filter(S, cases.GROW_M, 0.0, 0, 1), dtype=np.float64)
        pos, _ = sim_ref.argmax_margin(filtered)
        assert pos == want_pos, (name, pos)
        got = cases.walk(filtered, pos[0], pos[1], cases.GROW_M)
        assert got[1:] == (back, fwd, ties, stop), (name, got)
        assert got[0] == aS._grow_thumbnail(filtered, pos[0], pos[1], cases.GROW_M), name
        assert any(stop) or got[0][1] - got[0][0] == cases.GROW_M
        seen.add(stop)
    # each of the four conditions ends a walk, and a walk reaches m_filter cells
    assert {s[0] for s in seen} == {s[1] for s in seen} == {s[2] for s in seen} == {s[3] for s in seen} == {False, True}
    assert (False,) * 4 in seen
    S = cases.symmetric_matrix(65, 3)
    assert np.array_equal(S, S.T) and np.all(np.diag(S) == 1.0) and np.abs(S).max() <= 1.0
