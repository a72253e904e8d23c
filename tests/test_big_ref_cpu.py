"""The HBM-pass path without a device: tests/big_ref.py (the NumPy restatement of csrc/kernels_big.hpp) reproduces the oracle's spectrum
from the library's own radix schedule; the record of WHY tests/test_big_kernel_gpu.py runs the windows it runs (one-token mistakes in the
general-radix pass that a prime window cannot see); paa_debug_big_plan against hand-counted chunk sizes; and the signals of that file stay
inside assert_parity's default ill-conditioning budget, as tests/test_clip_edges_signals_cpu.py shows for its signals."""
import functools

import numpy as np
import pytest

import big_ref
import paa_oracle as O
from checks import ill_info
from pyaudioanalysis_amd import _ffi
from test_big_kernel_gpu import (EVEN, SCHEDULES, SEAM, SEAM_SPEC, WG_SEAMS, chroma_seam_signal, chunk_frames, feature_seam_signal,
                                 periodic_steps, ragged_batch, schedule_clip, schedule_step, seam_clip, seam_frames, spec_seam_signal)

COMPOSITE = [s[1] for s in SCHEDULES]
PRIME = 9001


def frame_of(window):
    return np.random.default_rng(window).standard_normal(window)


@pytest.mark.parametrize("fs,window,radices", SCHEDULES + [(16000, PRIME, [PRIME]), (16000, 80000, [4, 4, 4, 5, 5, 5, 5])],
                         ids=[str(w) for w in COMPOSITE + [PRIME, 80000]])
def test_hbm_passes_reproduce_the_spectrum(fs, window, radices):
    """the library's schedule is the one the GPU test names, and pass by pass -- templated and general form, even recombination / odd
    magnitude -- it gives the oracle's magnitude spectrum (every output written: the restatement starts from NaN)"""
    got_radices, Nc = big_ref.plan(window)
    assert got_radices == radices and Nc == (window // 2 if window % 2 == 0 else window)
    x = frame_of(window)
    ref = O.magnitude_spectrum(x, window // 2)
    got = big_ref.magnitude_spectrum(x)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    # two float64 transforms of the same frame: each within a few eps log2(N) of the exact spectrum, the 9001-term double sums of the
    # prime window within eps sqrt(9001) ~ 2e-14 (measured: 3e-16 .. 9e-16 of the peak, 5e-15 at 9001)
    assert np.abs(got - ref).max() <= 1e-13 * ref.max()


@functools.lru_cache(maxsize=None)
def good_spectrum(window):
    out = big_ref.magnitude_spectrum(frame_of(window))
    out.setflags(write=False)
    return out


def changed(got, ref):
    """largest change relative to the peak; an output the wrong index never wrote counts as changed"""
    d = np.abs(got - ref)
    d[np.isnan(d)] = np.inf
    return d.max() / ref.max()


def last_general_pass_only(radices):
    return all(r in big_ref.TEMPLATED for r in radices[:-1])


@pytest.mark.parametrize("mistake", big_ref.MISTAKES)
def test_one_token_mistakes_show_at_the_composite_windows_only(mistake):
    """Why the GPU test's windows: each one-token slip of big_pass_kernel's general branch moves the spectrum of every composite window of
    SCHEDULES by more than 1e-3 of its peak (measured: 0.7 .. 1.0) and the spectrum of the prime 9001 by NOTHING -- there Ns = 1, nb = 1,
    a = 1, k = 0 and both expressions collapse to q.
    One exception, by algebra: the output stride q*nb for q*Ns is the same expression in a plan's LAST pass (Ns R = Nc, so nb = Nc / R =
    Ns).  Windows whose only general pass is the last one (5472, 5508, 5463) cannot see that slip -- asserted as such, bit for bit; the
    four windows with a general pass in front of the last one (5474, 5491, 5510, 16537) do."""
    assert np.array_equal(big_ref.magnitude_spectrum(frame_of(PRIME), mistake), good_spectrum(PRIME))
    seen = []
    for _, window, radices in SCHEDULES:
        good, bad = good_spectrum(window), big_ref.magnitude_spectrum(frame_of(window), mistake)
        if mistake == "out_q_nb" and last_general_pass_only(radices):
            assert np.array_equal(good, bad), window
            continue
        assert changed(bad, good) > 1e-3, (mistake, window, changed(bad, good))
        seen.append(window)
    assert seen == COMPOSITE if mistake != "out_q_nb" else seen == [5474, 5491, 5510, 16537]


def test_chunk_sizes_against_hand_counts():
    """C = min(2^30 / (Nc 32 + Nf 8 + 24), 65 535, frames of the longest clip); the frame-list cap max(2, 2^30 / (Nf 8))"""
    for window, C in ((5491, 5431), (5474, 9805), (16537, 1803), (9001, 3313), (80000, 671)):
        p = big_ref.big_plan(window, 1 << 40)
        assert p["C"] == C, (window, p)
        assert p["Nc"] == (window // 2 if window % 2 == 0 else window) and p["Nf"] == window // 2 and p["even"] == 1 - window % 2
        assert p["per_frame"] == p["Nc"] * 32 + p["Nf"] * 8 + 24 and p["passes"] == len(big_ref.plan(window)[0])
        assert p["need"] == C * p["Nc"] * 32 + (C + 1) * p["Nf"] * 8 + C * 24 + 256 and p["need"] <= (1 << 30) + p["Nf"] * 8 + 256
        assert (C + 1) * p["per_frame"] > 1 << 30 >= C * p["per_frame"]
        # the clamp to the longest clip
        for frames in (1, 7, C - 1, C, C + 1):
            assert big_ref.big_plan(window, frames)["C"] == min(frames, C)
    for window, cap in ((6174, 43478), (11025, 24350)):
        assert big_ref.big_plan(window, 1)["wg_cap"] == cap
    # gridDim.y: a small window's budget holds more frames than a launch has rows
    assert big_ref.big_plan(64, 1 << 40)["C"] == 65535 and big_ref.big_plan(64, 65534)["C"] == 65534
    assert big_ref.big_plan(3, 1 << 40)["wg_cap"] == (1 << 30) // 8


def test_big_plan_refuses_bad_arguments():
    lib = _ffi.lib()
    assert "paa_debug_big_plan" in _ffi.EXPORTED_SYMBOLS
    info = np.zeros(8, dtype=np.int64)
    assert lib.paa_debug_big_plan(5491, 1, _ffi.as_i64p(info)) == _ffi.PAA_OK
    assert lib.paa_debug_big_plan(1, 1, _ffi.as_i64p(info)) == _ffi.ERR_ARG
    assert lib.paa_debug_big_plan(-5491, 1, _ffi.as_i64p(info)) == _ffi.ERR_ARG
    assert lib.paa_debug_big_plan(5491, 0, _ffi.as_i64p(info)) == _ffi.ERR_ARG
    assert lib.paa_debug_big_plan(5491, -3, _ffi.as_i64p(info)) == _ffi.ERR_ARG
    assert lib.paa_debug_big_plan(5491, 1, None) == _ffi.ERR_ARG


def test_no_window_of_the_gpu_test_is_a_bluestein_window():
    """(what can be said about the kernel choice without a device: the Bluestein kernel ends at 5 462 samples)"""
    lib = _ffi.lib()
    info, off = np.zeros(8, dtype=np.int32), np.zeros(3, dtype=np.int32)
    blu = lambda w: lib.paa_debug_blu_plan(w, 16000.0, info.ctypes.data_as(_ffi.c_i32p), off.ctypes.data_as(_ffi.c_i32p), None, 0)      # noqa: E731
    assert blu(5461) > 0
    for window in COMPOSITE + [PRIME]:
        assert blu(window) == 0, window


@pytest.mark.parametrize("fs,window,radices", SCHEDULES, ids=[str(w) for w in COMPOSITE])
def test_schedule_clips_stay_inside_the_default_budget(fs, window, radices):
    info = ill_info(schedule_clip(fs, window), fs, window, schedule_step(window))
    assert len(info.mask) == 7 and info.budget_ok(), info.counts()
    assert not info.other.any()          # (no frame that is flagged but not silent)


def test_ragged_batch_clips_stay_inside_the_default_budget():
    fs, W = EVEN
    clips, S = ragged_batch()
    infos = [ill_info(c, fs, W, S) for c in clips]
    assert [len(i.mask) for i in infos] == [1, 1, 5, 40]
    assert all(i.budget_ok() for i in infos), [i.counts() for i in infos]
    assert infos[0].silent.all() and infos[1].silent.all() and len(set(clips[0])) == 1 and not clips[1].any()


@pytest.mark.parametrize("extra", [1, 9])
def test_feature_seam_clips_stay_inside_the_default_budget(extra):
    """... and have no silent frame at all: a wrong carry across the seam cannot hide behind a flux of zero"""
    fs, W, S = SEAM
    x = feature_seam_signal(extra)
    C = chunk_frames(W, 1 << 40)
    info = ill_info(x, fs, W, S)
    assert len(info.mask) == seam_frames(extra) == C + extra
    assert info.budget_ok() and not info.silent.any() and not info.other.any(), info.counts()
    short = seam_clip(5493, W + 49 * S, fs)
    assert ill_info(short, fs, W, S).budget_ok()


def test_mode_seam_clips_are_what_the_gpu_test_says():
    """the chromagram seam clip: C + 9 full frames and a truncated tail the reference accepts (at least num_fft samples, fewer than a window);
    the spectrogram seam clip: C + 7 frames; the frame-list seam clips: a period longer than the window"""
    fs, W, _ = SEAM
    x, S, T = chroma_seam_signal()
    tail = len(x) - (W + T * S)
    assert T == chunk_frames(W, 1 << 40) + 9 and W // 2 <= tail < W and len(range(W, len(x) - S, S)) == T + 1
    assert len(x) - (W + (T - 1) * S) >= W
    fs, W, S = SEAM_SPEC
    x, T = spec_seam_signal()
    assert T == chunk_frames(W, 1 << 40) + 7 and len(range(W, len(x) - W + 1, S)) == T
    for fs, window, _, _ in WG_SEAMS:
        assert periodic_steps(window, 2) * 2 > window and periodic_steps(window, 2) % 7 == 0
