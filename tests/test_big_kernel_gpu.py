"""The HBM-pass kernels (csrc/kernels_big.hpp, run_big in csrc/lib_plan.hpp) on COMPOSITE windows, and the scratch seams of run_big and
of wg_build_work (csrc/lib_dispatch.hpp) under wg_lds / wg_split, against the NumPy oracle through the C ABI.  -m gpu.

Why these windows: at a prime window (9001, what the other suites run this path at) the plan is one general-radix pass with Ns = 1,
nb = 1, a = 1, k = 0, and the twiddle step and output index of big_pass_kernel collapse to q -- three one-token mistakes in them compute
the right answer there (tests/test_big_ref_cpu.py::test_one_token_mistakes_show_at_the_composite_windows_only).  SCHEDULES runs every
templated instance (2, 3, 4, 5) at Ns = 1 and Ns > 1, general passes at Ns > 1 first / in the middle / last, on even and odd windows.

The seams: run_big cuts a clip into chunks of C frames (C from the library: paa_debug_big_plan) and carries the last spectrum row of a
chunk into row 0 of the next (the flux of the chunk's first frame reads it); wg_build_work cuts the frame list at `wg_cap` frames and
starts the next chunk with a halo record.  Every seam case is a test of its own and asserts T > C with the library's number.

No tolerance of this file's own: comparisons go through test_parity_gpu.assert_parity with its defaults; the one exception is the bound
of tests/test_wgs_kernel_gpu.py::test_more_frames_than_one_chunk_of_the_scratch on the columns around the wg seams (WGS_SEAM_BOUND)."""
import functools

import numpy as np
import pytest

import big_ref
import checks
import paa_oracle as O
from pyaudioanalysis_amd import ShortTermFeatures, _ffi
from synth import synth_clip
from test_ct_kernels_gpu import make_signal
from test_parity_gpu import assert_parity, tight_violations

pytestmark = pytest.mark.gpu

HBM = "big_window_hbm_passes"
WGS_SEAM_BOUND = dict(rtol=1e-9, atol=1e-10)         # tests/test_wgs_kernel_gpu.py: the columns around its seam against O.frame_vector

# (fs, window, radices of the library's plan): what each one runs is in the comment
SCHEDULES = [
    (16000, 5474, [7, 17, 23]),               # even: three general passes, Ns = 1, 7, 119; even recombination
    (16000, 5491, [17, 17, 19]),              # odd: three general passes
    (16000, 5472, [4, 4, 3, 3, 19]),          # templated passes, then a general pass at Ns = 144
    (16000, 5508, [2, 3, 3, 3, 3, 17]),       # <2> at Ns = 1, <3> at Ns > 1
    (16000, 5510, [5, 19, 29]),               # <5> first, then two general passes
    (16000, 5463, [3, 3, 607]),               # odd: a long general radix at Ns = 9
    (11025, 16537, [23, 719]),                # odd: a 1.5 s window as users write it (1.5 * 11025 = 16537.5)
]
EVEN = (16000, 5474)                          # part B: modes, sample types, batches on an even composite window
SEAM = (16000, 5491, 8)                       # part C: fs, window, step of the features / chromagram seams
SEAM_SPEC = (11025, 16537, 8)                 # ... of the spectrogram seam (an odd window: 8 268 bins per row)
WG_SEAMS = [(16000, 6174, "st_wg_lds_fft", 0), (44100, 11025, "st_wg_split_fft", 3)]          # part D: fs, window, kernel, r0


def schedule_step(window):
    return window // 2 + 3


def schedule_clip(fs, window):
    """seven frames of synth_clip at the step of part A"""
    return synth_clip(5100 + window, window + 6 * schedule_step(window), fs)


def seam_clip(seed, n, fs):
    """Gaussian noise of amplitude 3000 plus two tones: no silent stretch (synth_clip has one, and the flux of two silent frames is 0
    whatever the carried row holds)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    x = 3000.0 * rng.standard_normal(n) + 4000.0 * np.sin(2.0 * np.pi * 440.0 * t) + 2500.0 * np.sin(2.0 * np.pi * 1730.5 * t + 1.0)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def chunk_frames(window, frames):
    """C of a run_big plan whose longest clip has `frames` frames, from the library"""
    return big_ref.big_plan(window, frames)["C"]


def seam_frames(extra):
    """C + extra frames at SEAM"""
    return chunk_frames(SEAM[1], 1 << 40) + extra


def feature_seam_signal(extra):
    fs, W, S = SEAM
    return seam_clip(5491 + extra, W + (seam_frames(extra) - 1) * S, fs)


@functools.lru_cache(maxsize=None)
def feature_seam_case(extra):
    """-> (clip of C + extra frames, oracle matrix with deltas, IllInfo); shared by the tests that run this clip, never written to"""
    fs, W, S = SEAM
    x = feature_seam_signal(extra)
    ref, _ = O.feature_extraction(x, fs, W, S, True)
    ref.setflags(write=False)
    return x, ref, checks.ill_info(x, fs, W, S)


def chroma_seam_signal():
    """C + 9 full frames at SEAM's window and a truncated tail frame.  The step is schedule_step(window), not SEAM's 8: chromagram() FFTs
    every truncated frame down to the last one (p < n - step), and the reference raises ValueError when that one is shorter than num_fft
    (ShortTermFeatures.py:288) -- with a step below num_fft / 2 it always is."""
    fs, W, _ = SEAM
    S = schedule_step(W)
    T = seam_frames(9)
    return seam_clip(5492, W + T * S + S + 100, fs), S, T          # frames start at W + i S; frame T has S + 100 samples left


def spec_seam_signal():
    fs, W, S = SEAM_SPEC
    T = chunk_frames(W, 1 << 40) + 7
    return seam_clip(16537, 2 * W + (T - 1) * S, fs), T            # frame i starts at W + i S


def periodic_steps(window, step):
    """7 x 2^k steps, the shortest such period longer than the window"""
    p = 7
    while p * step <= window:
        p *= 2
    return p


def wg_seam_signal(fs, window, step=2):
    """-> (clip, frames T = wg_cap + 60, period in steps).  The wgs seam test's clip is periodic in 7 steps of half a window; at a step
    of 2 samples seven steps are 14 samples, every frame would be that pattern 441 times over, and the reference's own MFCCs on its empty
    mel bands a function of round-off.  So the period is 7 x 2^k steps, longer than the window: a frame is plain noise, and frames one
    period apart still see the same samples and the same clip constants."""
    T = big_ref.big_plan(window, 1)["wg_cap"] + 60
    period = periodic_steps(window, step)
    n = window + (T - 1) * step
    block = (np.random.default_rng(window).standard_normal(period * step) * 3000).astype(np.int16)
    return np.tile(block, n // len(block) + 1)[:n], T, period


def ragged_batch():
    """four int16 clips of W, W + S - 1, 3 W + 17 samples and 40 frames at EVEN; the first a constant, the second digital silence"""
    fs, W = EVEN
    S = schedule_step(W)
    lens = [W, W + S - 1, 3 * W + 17, W + 39 * S]
    clips = [synth_clip(5200 + i, n, fs) for i, n in enumerate(lens)]
    clips[0] = np.full(lens[0], 1234, dtype=np.int16)
    clips[1] = np.zeros(lens[1], dtype=np.int16)
    return clips, S


def even_mode_signal(kind):
    """-> (signal as passed, mono): 7 full frames of EVEN's window behind the first and a truncated chromagram tail of S + 100 samples"""
    fs, W = EVEN
    S = schedule_step(W)
    n = W + 8 * S + 100
    sig, mono = make_signal(kind, 5300 + len(kind), (n + 0.5) / fs, fs)
    assert len(mono) == n
    return sig, mono, S


def kernel_of(fs, window, step, kind=0, mode=0, frames=4):
    plan = _ffi.Plan(np.array([0, 2 * window + frames * step], dtype=np.int64), fs, window, step, deltas=False, sample_kind=kind, mode=mode)
    try:
        return plan.kernel_name
    finally:
        plan.destroy()


def assert_deltas(got):
    assert np.array_equal(got[34:, 1:], got[:34, 1:] - got[:34, :-1]) and np.all(got[34:, 0] == 0.0)


def assert_carry_is_visible(x, fs, W, S, C, ref):
    """Before the kernel runs: the frames around the seam are not silent, and the oracle's flux at column C formed with a wrong previous
    frame -- C - 2 (a stale row), or none (the frame itself, as at t = 0) -- is further from the true value than ten times what assert_parity
    allows that entry: a tenth of the error is put on the reference matrix and its tight gate asked."""
    assert not checks.silent_mask(x, W, S)[C - 2:C + 3].any()
    xn = O.normalize_clip(x)
    tab = O.Tables(fs, W)
    spec = lambda t: O.magnitude_spectrum(xn[t * S:t * S + W], tab.nfft)          # noqa: E731
    X = spec(C)
    for X_wrong in (spec(C - 2), X):
        wrong = O.frame_vector(xn[C * S:C * S + W], X, X_wrong, tab)[6]
        probe = ref.copy()
        probe[6, C] += (wrong - ref[6, C]) / 10.0
        assert tight_violations(probe, ref)[1][6, C], (wrong, ref[6, C])


# ---- A. radix schedules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,window,radices", SCHEDULES, ids=[str(s[1]) for s in SCHEDULES])
def test_radix_schedules(gpu_lib, fs, window, radices):
    S = schedule_step(window)
    assert kernel_of(fs, window, S) == HBM
    assert big_ref.plan(window)[0] == radices
    x = schedule_clip(fs, window)
    ref, _ = O.feature_extraction(x, fs, window, S, True)
    got, _ = ShortTermFeatures.feature_extraction(x, fs, window, S, True)
    assert ref.shape == (68, 7)
    assert_parity(got, ref, "%d/%d@%d" % (window, S, fs), sig=(x, fs, window, S))
    assert_deltas(got)


# ---- B. modes, sample types and batches on an even composite window ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["i16", "f64", "stereo"])
def test_even_window_spectrogram_and_chromagram(gpu_lib, capsys, kind):
    fs, W = EVEN
    sig, mono, S = even_mode_signal(kind)
    code = {"i16": 0, "f64": 1, "stereo": 2}[kind]
    assert kernel_of(fs, W, S, kind=code, mode=1) == HBM and kernel_of(fs, W, S, kind=code, mode=2) == HBM
    spec, t_ax, f_ax = ShortTermFeatures.spectrogram(sig, fs, W, S)
    capsys.readouterr()
    ref, _, _ = O.spectrogram(mono, fs, W, S)
    assert spec.shape == ref.shape and len(f_ax) == W // 2 and len(t_ax) == ref.shape[0]
    assert_parity(np.ascontiguousarray(spec.T), np.ascontiguousarray(ref.T), "spectrogram %s %d/%d" % (kind, W, S))
    cref, _, _ = O.chromagram(mono, fs, W, S)
    chroma, _, names = ShortTermFeatures.chromagram(sig, fs, W, S)
    assert chroma.shape == cref.shape == (8, 12) and names == O.CHROMA_NAMES          # 7 full frames and the truncated tail
    assert len(mono) - (W + 7 * S) == S + 100 < W
    assert_parity(np.ascontiguousarray(chroma.T), np.ascontiguousarray(cref.T), "chromagram %s %d/%d" % (kind, W, S))


def test_even_window_ragged_batch(gpu_lib):
    """One plan for four clips (a clip of exactly one window, one a sample short of a second frame, a constant one and a digitally silent
    one among them): bit-identical to the single-clip calls, each clip against the oracle."""
    fs, W = EVEN
    clips, S = ragged_batch()
    assert kernel_of(fs, W, S) == HBM
    res, _ = ShortTermFeatures.feature_extraction_batch(clips, fs, W, S, deltas=True)
    assert [r.shape[1] for r in res] == [1, 1, 5, 40]
    for c, r in zip(clips, res):
        single, _ = ShortTermFeatures.feature_extraction(c, fs, W, S)
        assert np.array_equal(single, r)
        ref, _ = O.feature_extraction(c, fs, W, S)
        assert_parity(r, ref, "ragged batch at %d" % W, sig=(c, fs, W, S))
        assert_deltas(r)


# ---- C. the seam of run_big ------------------------------------------------------------------------------------------------------
def run_feature_seam(extra):
    fs, W, S = SEAM
    x, ref, info = feature_seam_case(extra)
    T = ref.shape[1]
    C = chunk_frames(W, T)
    assert T == C + extra and T > C
    assert kernel_of(fs, W, S) == HBM
    assert_carry_is_visible(x, fs, W, S, C, ref)
    got, _ = ShortTermFeatures.feature_extraction(x, fs, W, S, True)
    assert_parity(got, ref, "%d/%d, %d frames in chunks of %d" % (W, S, T, C), ill=info)
    assert_deltas(got)


def test_seam_last_chunk_of_one_frame(gpu_lib):
    """T = C + 1: the second chunk is one frame, whose flux reads the carried row and whose deltas reach across the seam"""
    run_feature_seam(1)


def test_seam_last_chunk_of_nine_frames(gpu_lib):
    run_feature_seam(9)


def test_seam_in_the_second_clip_of_a_batch(gpu_lib):
    """C comes from the longest clip; the first clip ends inside a chunk, the second (test_seam_last_chunk_of_nine_frames's clip) crosses the
    seam with the scratch the first one left behind"""
    fs, W, S = SEAM
    x, ref, info = feature_seam_case(9)
    short = seam_clip(5493, W + 49 * S, fs)
    T = ref.shape[1]
    C = chunk_frames(W, T)
    assert T > C > 50 and kernel_of(fs, W, S) == HBM
    res, _ = ShortTermFeatures.feature_extraction_batch([short, x], fs, W, S, deltas=True)
    assert res[0].shape == (68, 50) and res[1].shape == ref.shape
    ref0, _ = O.feature_extraction(short, fs, W, S)
    assert_parity(res[0], ref0, "first clip of the seam batch", sig=(short, fs, W, S))
    assert_parity(res[1], ref, "second clip of the seam batch", ill=info)
    assert_deltas(res[1])


def test_seam_chromagram(gpu_lib):
    fs, W, _ = SEAM
    x, S, T = chroma_seam_signal()
    C = chunk_frames(W, T)
    assert T == C + 9 and T > C and kernel_of(fs, W, S, mode=2) == HBM
    assert len(range(W, len(x) - S, S)) == T + 1 and len(x) - (W + T * S) == S + 100          # T full frames and the tail
    assert not checks.silent_mask(x[W:], W, S)[C - 2:C + 3].any()
    ref, _, _ = O.chromagram(x, fs, W, S)
    got, _, _ = ShortTermFeatures.chromagram(x, fs, W, S)
    assert got.shape == ref.shape == (T + 1, 12)
    assert_parity(np.ascontiguousarray(got.T), np.ascontiguousarray(ref.T), "chromagram %d/%d, %d frames in chunks of %d" % (W, S, T, C))


def test_seam_spectrogram(gpu_lib, capsys):
    """spectrogram mode writes the rows of a chunk straight to the output at row0 = t0"""
    fs, W, S = SEAM_SPEC
    x, T = spec_seam_signal()
    C = chunk_frames(W, T)
    assert T == C + 7 and T > C and kernel_of(fs, W, S, mode=1) == HBM
    assert len(range(W, len(x) - W + 1, S)) == T
    assert not checks.silent_mask(x[W:], W, S)[C - 2:C + 3].any()
    ref, _, _ = O.spectrogram(x, fs, W, S)
    got, _, _ = ShortTermFeatures.spectrogram(x, fs, W, S)
    capsys.readouterr()
    # (the reference allocates int((n - W) / S) + 1 rows and fills T of them: the rest stay zero and are compared as such)
    assert got.shape == ref.shape and ref.shape[0] > T and not got[T:].any() and not ref[T:].any()
    assert_parity(np.ascontiguousarray(got[:T].T), np.ascontiguousarray(ref[:T].T), "spectrogram %d/%d, %d frames in chunks of %d" % (W, S, T, C))


# ---- D. the seam of wg_build_work under wg_lds and wg_split ------------------------------------------------------------------------
@pytest.mark.parametrize("fs,window,kernel,r0", WG_SEAMS, ids=[w[2] for w in WG_SEAMS])
def test_seam_of_the_frame_list(gpu_lib, fs, window, kernel, r0):
    """More frames than one chunk of the frame list holds: the second chunk starts with a halo record (and, split transforms, has a task
    list of its own, pairs first).  Columns one period apart are bit-identical across the seam; the columns around it against the oracle."""
    S = 2
    x, T, period = wg_seam_signal(fs, window, S)
    cap = big_ref.big_plan(window, T)["wg_cap"]
    assert T == cap + 60 and T > cap and period * S > window and 2 * period < cap - 2
    assert kernel_of(fs, window, S) == kernel
    info = np.zeros(48, dtype=np.int32)
    assert gpu_lib.paa_debug_wg_plan(window, info.ctypes.data_as(_ffi.c_i32p), None, 0) == 1 and info[3] == r0
    F, _ = ShortTermFeatures.feature_extraction(x, fs, window, S, deltas=False)
    assert F.shape == (34, T)
    assert np.array_equal(F[:, period:T - period], F[:, 2 * period:T])          # (column 0 has flux 0: the comparison starts one period in)
    again, _ = ShortTermFeatures.feature_extraction(x, fs, window, S, deltas=False)
    assert np.array_equal(F, again)
    xn = O.normalize_clip(x)
    tab = O.Tables(fs, window)
    for t in range(cap - 2, cap + 3):
        fr = xn[t * S:t * S + window]
        v = O.frame_vector(fr, O.magnitude_spectrum(fr, tab.nfft), O.magnitude_spectrum(xn[(t - 1) * S:(t - 1) * S + window], tab.nfft), tab)
        print("%s column %d (seam at %d): max |d| %.3g, max |d| / (atol + rtol |ref|) %.3g" % (
            kernel, t, cap, np.abs(F[:34, t] - v).max(),
            (np.abs(F[:34, t] - v) / (WGS_SEAM_BOUND["atol"] + WGS_SEAM_BOUND["rtol"] * np.abs(v))).max()))
        assert np.allclose(F[:34, t], v, **WGS_SEAM_BOUND), t
