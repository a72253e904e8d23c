"""Clips at the edges of the clip constants (csrc/device_common.hpp: ClipNorm) through every feature-kernel family, against the
oracle through assert_parity with its default allowances (ZCR and roll-off: zero flips).  -m gpu.

* The one-wave families fold the statistics partials in their own prologue (wave_clip_norm, norms_inline = 1) and never run
  clip_params_kernel: long clips whose loud part and DC offset sit in the LAST statistics chunk only, at 257 chunks (features,
  second clip of a batch: stat_first > 0) and 193 chunks (spectrogram), the two chunk counts at which clip_norm_wave's loops hand
  over.  A missed partial changes inv, and with it the energy row, by orders of magnitude.
* Rail clips: a seeded random telegraph signal between -32768 and 32767 that sits on one rail 85 % of the time (random dwell
  times: a broadband spectrum).  Its mean lies near -+23000 counts, so x - m_int reaches 55000 -- beyond 2^15, where no
  full-scale square wave (mean ~ 0) gets.
* On the mean: test_mix_kernel_gpu.py::test_samples_that_sit_on_a_whole_number_mean's mirrored clip (a whole-number mean with a
  fifth of the samples on it) for the families that test does not list.
* Degenerate clips (zeros, constant DC, exactly one window, W + S - 1 samples, silence inside) for wgs, wg_lds, wg_split, the
  passes through HBM and generic, after test_ct_kernels_gpu.py::test_degenerate_clips_through_the_family.  No Nyquist square
  wave, for the reason test_mix_kernel_gpu.py gives.

One shape per family, the smallest windows tests/test_tile_launch_gpu.py and test_parity_gpu.py::test_big_window_kernel_choice
name; the kernel name is asserted first.  st_generic takes only windows for which the reference has no feature matrix (fewer
than 64 bins: see test_tile_launch_gpu.py), so it runs its spectrogram rows here.  tests/test_clip_edges_signals_cpu.py checks,
without a device, that every signal here stays inside the default ill-conditioning budget."""
import functools

import numpy as np
import pytest

import paa_oracle as O
from checks import ill_info, reference_matrix
from pyaudioanalysis_amd import ShortTermFeatures, _ffi
from synth import synth_clip
from test_parity_gpu import assert_parity

pytestmark = pytest.mark.gpu

KINDS = ("i16", "f64", "stereo")
# family rung -> (fs, window, step, kernel name, sample types)
SHAPES = {
    "fast": (16000, 800, 400, "st_fast_800_w8", ("i16",)),
    "ct": (16000, 320, 160, "st_ct_10x16", KINDS),
    "tri_551": (11025, 551, 275, "st_tri_r29x19", KINDS),
    "tri_2205": (44100, 2205, 1102, "st_tri_r21x21x5", KINDS),
    "mix": (44100, 4096, 2048, "st_mix", KINDS),
    "blu": (22050, 661, 220, "st_blu_1024", KINDS),
    "generic": (8000, 100, 50, "spectrogram_generic", KINDS),
    "wgr": (8000, 8000, 4000, "st_wgr_10x20x20", KINDS),
    "wgs_6": (22050, 22050, 11025, "st_wgs_6x3675", KINDS),
    "wgs_12": (44100, 44100, 22050, "st_wgs_12x3675", KINDS),
    "wg_lds": (16000, 9009, 4505, "st_wg_lds_fft", KINDS),
    "wg_split": (44100, 11025, 5513, "st_wg_split_fft", KINDS),
    "hbm": (16000, 9001, 4501, "big_window_hbm_passes", KINDS),
}
CASES = [(r, k) for r, sh in SHAPES.items() for k in sh[4]]
# the families test_samples_that_sit_on_a_whole_number_mean does not list (generic has no zero-crossing row: spectrogram only)
ON_MEAN = [(r, k) for r in ("mix", "blu", "wgr", "wgs_6", "wgs_12", "wg_lds", "wg_split", "hbm") for k in KINDS]
DEGENERATE = ("generic", "wgs_6", "wgs_12", "wg_lds", "wg_split", "hbm")


def kernel_name(rung, kind, n):
    fs, window, step, _, _ = SHAPES[rung]
    plan = _ffi.Plan(np.array([0, n], dtype=np.int64), fs, window, step, deltas=False, sample_kind=KINDS.index(kind),
                     mode=1 if rung == "generic" else 0)
    try:
        return plan.kernel_name
    finally:
        plan.destroy()


def views(stereo, kind):
    """-> (what the library gets, the mono signal the oracle gets) of an (n, 2) int16 clip: its left channel, the reference's
    float64 downmix, or the interleaved frames (summed on the device)"""
    if kind == "i16":
        left = np.ascontiguousarray(stereo[:, 0])
        return left, left
    mono = O.stereo_to_mono(stereo)
    return (stereo, mono) if kind == "stereo" else (mono, mono)


def telegraph(seed, n, low_share=0.85):
    """(n, 2) int16: per channel a random telegraph signal between the rails that sits on the negative one `low_share` of the
    time; dwell times are geometric (mean 17 samples low, 3 high at 0.85), so the spectrum is broadband"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 2), dtype=np.int16)
    for c in range(2):
        pairs = n // 16 + 8
        low = rng.geometric(1.0 / (20.0 * low_share), pairs)
        high = rng.geometric(1.0 / (20.0 * (1.0 - low_share)), pairs)
        runs = np.stack([low, high], axis=1).reshape(-1)
        level = np.tile(np.array([-32768, 32767], dtype=np.int16), pairs)
        x = np.repeat(level, runs)
        while len(x) < n:
            x = np.concatenate([x, x])
        out[:, c] = x[:n]
    return out


@functools.lru_cache(maxsize=None)
def rail_clip(rung, mirrored):
    fs, window, step, _, _ = SHAPES[rung]
    x = telegraph(3100 + sorted(SHAPES).index(rung), 5 * window + 3)
    return (-1 - x) if mirrored else x          # (-1 - x: the mirror image of an int16 signal, -32768 <-> 32767)


def mirrored_clip(rung):
    """(a, -a) + c per channel: L has the whole-number mean 40, R -27 (L + R: 13, the downmix 6.5), a fifth of the samples on it"""
    fs, window, step, _, _ = SHAPES[rung]
    rng = np.random.default_rng(3200 + sorted(SHAPES).index(rung))
    n = 3 * window

    def half(c, amp):
        a = rng.integers(-amp, amp + 1, n)
        a[rng.random(n) < 0.2] = 0
        return np.concatenate([a, -a]) + c
    return np.stack([half(40, 2500), half(-27, 2500)], axis=1).astype(np.int16)


def run_and_check(rung, kind, stereo, what):
    fs, window, step, name, _ = SHAPES[rung]
    sig, mono = views(stereo, kind)
    assert kernel_name(rung, kind, len(stereo)) == name
    if rung == "generic":
        spec, _, _ = ShortTermFeatures.spectrogram(sig, fs, window, step)
        ref = O.spectrogram(mono, fs, window, step)[0]
        assert spec.shape == ref.shape
        assert_parity(np.ascontiguousarray(spec.T), np.ascontiguousarray(ref.T), what)
        return None, None
    F, _ = ShortTermFeatures.feature_extraction(sig, fs, window, step, False)
    ref = reference_matrix(mono, fs, window, step, False)
    assert_parity(F, ref, what, ill=ill_info(mono, fs, window, step))
    return F, ref


@pytest.mark.parametrize("rung,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_rail_bound_clips(gpu_lib, capsys, rung, kind):
    for mirrored in (False, True):
        stereo = rail_clip(rung, mirrored)
        mean = float(np.mean(views(stereo, kind)[1]))
        assert 19000 < abs(mean) < 27000 and (mean > 0) == mirrored
        run_and_check(rung, kind, stereo, "rail %s %s%s" % (rung, kind, " mirrored" if mirrored else ""))


@pytest.mark.parametrize("rung,kind", ON_MEAN, ids=["%s-%s" % c for c in ON_MEAN])
def test_samples_on_a_whole_number_mean(gpu_lib, rung, kind):
    fs, window, step, _, _ = SHAPES[rung]
    stereo = mirrored_clip(rung)
    mono = views(stereo, kind)[1]
    assert float(np.mean(np.double(mono) * (1.0 if kind == "i16" else 2.0))) in (40.0, 13.0)
    if kind == "i16":
        assert np.mean(mono == 40) > 0.15
    F, ref = run_and_check(rung, kind, stereo, "whole mean %s %s" % (rung, kind))
    counts = lambda row: np.rint(row * 2.0 * (window - 1))        # noqa: E731  zcr = sum |diff(sign)| / 2 / (W - 1): whole numbers
    assert np.array_equal(counts(F[0]), counts(ref[0])) and np.abs(F[0] * 2.0 * (window - 1) - counts(F[0])).max() < 1e-6


@pytest.mark.parametrize("rung", DEGENERATE)
def test_degenerate_clips(gpu_lib, capsys, rung):
    fs, W, S, name, _ = SHAPES[rung]
    seed = 3300 + 10 * sorted(SHAPES).index(rung)
    cases = {
        "zeros": np.zeros(5 * W, dtype=np.int16),
        "one_window": synth_clip(seed, W, fs),
        "w_plus_s_minus_1": synth_clip(seed + 1, W + S - 1, fs),
        "dc": np.full(4 * W, 1234, dtype=np.int16),
    }
    x = synth_clip(seed + 2, 6 * W, fs).copy()
    x[2 * W + 7:4 * W] = 0
    cases["silence_inside"] = x
    for label, sig in cases.items():
        if rung == "generic":
            if len(sig) < 2 * W + 1:          # (spectrogram frames start at sample W: shorter clips have none)
                sig = np.concatenate([sig, sig, sig[:S]])
            assert kernel_name(rung, "i16", len(sig)) == name
            spec, _, _ = ShortTermFeatures.spectrogram(sig, fs, W, S)
            ref = O.spectrogram(sig, fs, W, S)[0]
            assert spec.shape == ref.shape
            assert_parity(np.ascontiguousarray(spec.T), np.ascontiguousarray(ref.T), "%s %s" % (rung, label))
            continue
        assert kernel_name(rung, "i16", len(sig)) == name
        F, _ = ShortTermFeatures.feature_extraction(sig, fs, W, S)
        ref, _ = O.feature_extraction(sig, fs, W, S)
        assert_parity(F, ref, "%s %s" % (rung, label), sig=(sig, fs, W, S))
    if rung != "generic":
        with pytest.raises(ValueError):
            ShortTermFeatures.feature_extraction(synth_clip(seed + 3, W - 1, fs), fs, W, S)


# ---- the inline fold of the one-wave families ----------------------------------------------------------------------------------
CHUNK = 4096          # samples per statistics chunk of a short batch (csrc/lib_plan.hpp: stat_chunk_for)


@functools.lru_cache(maxsize=None)
def loud_last_chunk(seed, chunks):
    """int16 clip of `chunks` statistics chunks (the last one 100 samples short): a quiet tone in noise, and in the last chunk
    only a loud broadband part on a DC offset"""
    rng = np.random.default_rng(seed)
    n = chunks * CHUNK - 100
    t = np.arange(n)
    x = 60.0 * np.sin(2.0 * np.pi * 0.031 * t) + 25.0 * rng.standard_normal(n)
    a = (chunks - 1) * CHUNK
    x[a:] += 7000.0 + 6000.0 * rng.standard_normal(n - a)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def test_inline_fold_of_257_chunks_behind_another_clip(gpu_lib):
    fs, W, S = 16000, 320, 320
    clips = [synth_clip(3400, 3 * CHUNK - 17, fs), loud_last_chunk(3401, 257)]
    assert kernel_name("ct", "i16", len(clips[1])) == "st_ct_10x16" and sum(len(c) for c in clips) <= 1024 * CHUNK
    res, _ = ShortTermFeatures.feature_extraction_batch(clips, fs, W, S, deltas=False)
    for i, (c, r) in enumerate(zip(clips, res)):
        assert_parity(r, reference_matrix(c, fs, W, S, False), "inline fold, clip %d" % i, ill=ill_info(c, fs, W, S))
    assert res[1].shape[1] > 3280


def test_inline_fold_of_193_chunks_in_spectrogram_mode(gpu_lib, capsys):
    import c_oracle
    fs, W, S = 16000, 320, 320
    x = loud_last_chunk(3402, 193)
    plan = _ffi.Plan(np.array([0, len(x)], dtype=np.int64), fs, W, S, deltas=False, mode=1)
    name = plan.kernel_name
    plan.destroy()
    assert name == "spectrogram_ct_10x16"
    spec, _, _ = ShortTermFeatures.spectrogram(x, fs, W, S)
    ref = c_oracle.spectrogram(x, W, S)
    assert spec.shape == ref.shape and spec.shape[0] > 2400
    assert_parity(np.ascontiguousarray(spec.T), np.ascontiguousarray(ref.T), "inline fold, spectrogram")
