"""The per-frame feature phase of the 800-sample int16 kernel (kernels_fast.hpp), on clips of a handful of frames, against the
NumPy oracle under the tight gate of test_parity_gpu:

* the flux scale 1 / sum(X_prev + eps) is handed from frame to frame (group to group inside a quad, last group to first across
  iterations) instead of being summed again: clips of 1 .. 9 frames cross the group, quad and 8-frame store-chunk boundaries;
  two tilings of one clip must agree bit for bit; silence next to tones makes the handed-on value 1 / (400 eps) exactly;
* the roll-off scan works in two levels (chunk, then bin): two bin-exact tones put the crossing on chosen bins;
* the mel lists: one tone per filter centre, the edges of the longest filter, white noise.

Every test passes on the kernel before the hand-over / two-level scan as well: none of them states the new roll-off summation
order (the inputs keep the threshold away from every cumulative sum, test_rolloff_inputs_keep_the_threshold_clear).  -m gpu."""
import functools

import numpy as np
import pytest

import checks
import paa_oracle as O
from pyaudioanalysis_amd import ShortTermFeatures, _ffi
from synth import synth_clip
from test_parity_gpu import assert_parity

W = 800
FRAME_COUNTS = (1, 2, 3, 4, 5, 8, 9)


def n_samples(frames, step):
    return W + (frames - 1) * step


def tone(n, k, amp, fs_bins=W):
    """bin-exact sinusoid: k periods per 800 samples (k * 20 Hz at 16 kHz)"""
    return amp * np.sin(2.0 * np.pi * k * np.arange(n) / fs_bins)


def to_i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def gpu_and_ref(x, fs, step, deltas):
    got, _ = ShortTermFeatures.feature_extraction(x, fs, W, step, deltas)
    ref, _ = O.feature_extraction(x, fs, W, step, deltas)
    return got, ref


def assert_fast(fs, step, deltas, n):
    plan = _ffi.Plan(np.array([0, n], dtype=np.int64), fs, W, step, deltas=deltas)
    name = plan.kernel_name
    plan.destroy()
    assert "fast" in name, name


# ---------------------------------------------------------------- frame counts
@functools.lru_cache(maxsize=None)
def count_clips(step):
    return tuple(synth_clip(900 + f, n_samples(f, step)) for f in FRAME_COUNTS)


@pytest.mark.gpu
@pytest.mark.parametrize("deltas", [False, True])
@pytest.mark.parametrize("step", [400, 800])
def test_clips_of_a_handful_of_frames(gpu_lib, step, deltas):
    """1 .. 9 frames per clip, one by one and as one batch in one plan"""
    clips = count_clips(step)
    assert_fast(16000, step, deltas, clips[-1].size)
    batch, _ = ShortTermFeatures.feature_extraction_batch(list(clips), 16000, W, step, deltas)
    for f, x, b in zip(FRAME_COUNTS, clips, batch):
        got, ref = gpu_and_ref(x, 16000, step, deltas)
        assert got.shape == ((68 if deltas else 34), f)
        assert_parity(got, ref, "%d frames 800/%d deltas=%s" % (f, step, deltas), sig=(x, 16000, W, step))
        assert np.array_equal(got, b), "batch member of %d frames differs from the single clip" % f


# ---------------------------------------------------------------- tilings
@pytest.mark.gpu
@pytest.mark.parametrize("step", [400, 800])
def test_two_tilings_agree_bit_for_bit(gpu_lib, step):
    """A 70-frame clip is cut into runs of 16 frames; a run after the first starts its first quad one frame early without
    deltas and two frames early with them (runs at frames 16, 31, 46, 61 / 16, 30, 44, 58), so one frame sits in different
    groups of different quads in the two plans: frame 32 is group 2 of its run's first quad in one and group 0 of a second quad
    (scale handed across iterations) in the other.  The 34 base rows are the same numbers: identity, not a tolerance."""
    x = synth_clip(4242, n_samples(70, step))
    base, _ = ShortTermFeatures.feature_extraction(x, 16000, W, step, False)
    full, _ = ShortTermFeatures.feature_extraction(x, 16000, W, step, True)
    assert base.shape == (34, 70) and full.shape == (68, 70)
    assert np.array_equal(base, full[:34])
    ref, _ = O.feature_extraction(x, 16000, W, step, True)
    assert_parity(full, ref, "70 frames 800/%d" % step, sig=(x, 16000, W, step))


# ---------------------------------------------------------------- inputs of the handed-on flux scale
def carry_clip(kind, step):
    n = n_samples(9, step)
    x = np.zeros(n)
    cut = 4 * step + W                # frames 0 .. 4 lie before the cut (whole periods of the tone: its mean stays 0)
    if kind == "silence":
        pass
    elif kind == "silence_off_zero":
        x[:] = -1234
    elif kind == "silence_then_tone":
        x[cut:] = tone(n - cut, 37, 9000.0)
    elif kind == "tone_then_silence":
        x[:cut] = tone(cut, 37, 9000.0)
    elif kind == "square":
        x = np.where((np.arange(n) // 21) % 2 == 0, 32767, -32768)
    elif kind == "impulse":
        x[2 * step + 123] = 32767
    return to_i16(x)


CARRY_KINDS = ("silence", "silence_off_zero", "silence_then_tone", "tone_then_silence", "square", "impulse")


@pytest.mark.gpu
@pytest.mark.parametrize("deltas", [False, True])
@pytest.mark.parametrize("step", [400, 800])
@pytest.mark.parametrize("kind", CARRY_KINDS)
def test_flux_scale_inputs(gpu_lib, kind, step, deltas):
    x = carry_clip(kind, step)
    got, ref = gpu_and_ref(x, 16000, step, deltas)
    # pure tones and silence are line spectra: the reference's own MFCCs of those frames are round-off (the checker holds the
    # silent ones to the analytic vector instead); every other row, flux among them, stays under the tight gate
    assert_parity(got, ref, "%s 800/%d deltas=%s" % (kind, step, deltas), sig=(x, 16000, W, step), max_other_abs=9)
    if kind in ("silence_then_tone", "tone_then_silence"):
        # the clip mean is exactly 0, so the silent frames' spectra -- and the predecessor sums -- are exactly 0
        # (1 / (400 eps) is the scale of such a predecessor; the flux row is held to the oracle by the gate above)
        assert int(x.astype(np.int64).sum()) == 0
        silent = checks.silent_mask(x, W, step)
        assert silent.sum() >= 3 and not silent.all()


# ---------------------------------------------------------------- roll-off
# (k1, k2): the crossing lands on k1 when the lower tone holds 91 % of the energy and on k2 when it holds 89 %.  Positions inside
# a 5-bin chunk: 24 last, 25 first (the lane edge 24 | 25), 7 middle, 399 last (the last bin), 100 first, 104 last, 202 middle;
# k1 = 0 is the DC bin: a level instead of a tone (clip halves at +c and -c keep the clip mean at 0)
ROLLOFF_PAIRS = ((24, 25), (7, 399), (100, 104), (0, 202))
ROLLOFF_SHARES = (0.89, 0.91)


@functools.lru_cache(maxsize=None)
def rolloff_clip(k1, k2, share, step):
    frames = 4 if step == 800 else 5
    n = n_samples(frames, step)
    a = 12000.0
    hi = tone(n, k2, a * np.sqrt(1.0 - share))
    if k1 > 0:
        lo = tone(n, k1, a * np.sqrt(share))
    else:                              # |X[0]| = 2 c against |X[k]| = amplitude
        c = 0.5 * a * np.sqrt(share)
        lo = np.where(np.arange(n) < n // 2, c, -c)
    x = to_i16(lo + hi)
    x.setflags(write=False)
    return x


def rolloff_frames(x, step):
    """(crossing bin, relative distance of the threshold from the nearest cumulative sum) per frame, from the oracle's spectra"""
    xn = O.normalize_clip(x)
    out = []
    for pos in range(0, xn.size - W + 1, step):
        P = O.magnitude_spectrum(xn[pos:pos + W], W // 2) ** 2
        cum, thr = np.cumsum(P) + O.EPS, 0.90 * np.sum(P)
        out.append((int(np.nonzero(cum > thr)[0][0]), float(np.min(np.abs(cum - thr)) / thr)))
    return out


@pytest.mark.parametrize("step", [400, 800])
def test_rolloff_inputs_keep_the_threshold_clear(step):
    """CPU: no frame of the roll-off inputs puts 0.9 sum(X^2) within 1e-9 relative of a cumulative sum (so no case has to be
    excluded for a rounding tie), and the crossings are where the cases want them"""
    for k1, k2 in ROLLOFF_PAIRS:
        for share in ROLLOFF_SHARES:
            x = rolloff_clip(k1, k2, share, step)
            frames = rolloff_frames(x, step)
            assert min(m for _, m in frames) > 1e-9, (k1, k2, share, frames)
            want = k1 if share > 0.9 else k2
            hits = [b for b, _ in frames]
            if k1 > 0:
                assert hits == [want] * len(hits), (k1, k2, share, hits)
            else:                      # the frame that straddles the level change has a spectrum of its own
                assert hits.count(want) >= len(hits) - 1, (k1, k2, share, hits)


@pytest.mark.gpu
@pytest.mark.parametrize("step", [400, 800])
@pytest.mark.parametrize("share", ROLLOFF_SHARES)
@pytest.mark.parametrize("pair", ROLLOFF_PAIRS, ids=lambda p: "%d-%d" % p)
def test_rolloff_lands_on_the_oracle_bin(gpu_lib, pair, share, step):
    x = np.array(rolloff_clip(pair[0], pair[1], share, step))
    got, ref = gpu_and_ref(x, 16000, step, False)
    assert np.array_equal(got[7], ref[7]), (got[7] * 400, ref[7] * 400)          # zero flips
    assert np.array_equal(np.round(ref[7] * 400).astype(int), [b for b, _ in rolloff_frames(x, step)])
    assert_parity(got, ref, "roll-off %s %.2f 800/%d" % (pair, share, step), sig=(x, 16000, W, step), max_other_abs=got.shape[1])


# ---------------------------------------------------------------- mel lists
def mel_bins():
    """(bin of every filter's largest weight, first and last bin of the longest filter)"""
    bank = O.mel_bank(16000, W // 2)
    centres = [int(np.argmax(row)) for row in bank]
    longest = int(np.argmax((bank > 0).sum(axis=1)))
    nz = np.nonzero(bank[longest])[0]
    return centres, int(nz[0]), int(nz[-1])


@functools.lru_cache(maxsize=None)
def mel_clips():
    """three frames each: a tone over a seeded noise floor (far above round-off: every mel band stays well-conditioned)"""
    centres, first, last = mel_bins()
    n = n_samples(3, 400)
    clips = []
    for j, k in enumerate(centres + [first, last]):
        rng = np.random.default_rng(7000 + j)
        clips.append(to_i16(tone(n, k, 12000.0) + 300.0 * rng.standard_normal(n)))
    return tuple(clips)


@pytest.mark.gpu
def test_mel_filter_centres_and_edges(gpu_lib):
    clips = mel_clips()
    assert len(clips) == 42
    batch, _ = ShortTermFeatures.feature_extraction_batch(list(clips), 16000, W, 400, False)
    for j, (x, got) in enumerate(zip(clips, batch)):
        info = checks.ill_info(x, 16000, W, 400)
        assert not info.mask.any(), "tone %d: the noise floor does not keep the reference's MFCCs well-conditioned" % j
        ref, _ = O.feature_extraction(x, 16000, W, 400, False)
        assert_parity(got, ref, "mel tone %d" % j, ill=info)          # no exemption: MFCC rows under the tight gate


@pytest.mark.gpu
@pytest.mark.parametrize("deltas", [False, True])
def test_mel_white_noise(gpu_lib, deltas):
    rng = np.random.default_rng(20240)
    x = to_i16(4000.0 * rng.standard_normal(n_samples(9, 400)))
    info = checks.ill_info(x, 16000, W, 400)
    assert not info.mask.any()
    got, ref = gpu_and_ref(x, 16000, 400, deltas)
    assert_parity(got, ref, "white noise deltas=%s" % deltas, ill=info)


# ---------------------------------------------------------------- the other shape
@pytest.mark.gpu
def test_22050_hz_takes_the_run_time_lists(gpu_lib):
    """22.05 kHz: longer mel / chroma lists than the compile-time ones (the kernel's non-fixed instantiation)"""
    x = synth_clip(2205, n_samples(9, 400), 22050)
    assert_fast(22050, 400, True, x.size)
    got, ref = gpu_and_ref(x, 22050, 400, True)
    assert_parity(got, ref, "9 frames 800/400@22050", sig=(x, 22050, W, 400))
