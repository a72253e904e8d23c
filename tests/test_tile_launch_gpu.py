"""The launch path the one-wave families share (csrc/family_launch.hpp: TileArgs, tile_launch, with_sample_type): every rung
of every family's ladder -- family x mode x sample type -- is reached through a device-resident plan and stores the right
rows, and the raised LDS attribute is set again after paa_shutdown -> paa_init.  -m gpu.

One plan per rung, at the smallest window its family takes (read off the *_select functions): 800/400 and 800/800 int16 for
fast; 320 for ct; 1102, 551 and 256 for the three tri units; 200 for mix (100 = 2^2 5^2 complex points, no register
family); 346 = 2 x 173 for the packed and 661 for the unpacked Bluestein kernel; 100 for generic (fewer than 64 bins: neither
mix nor blu).  The reference itself has no features and no chromagram for a window that small (its chroma table needs about
99 bins), and from 64 bins on mix or blu take every window up to the 8192-point convolution, so generic runs its
spectrogram rung only -- its ladder has one kernel per sample type and no mode rung.  Steps are at least half a window, so
that a truncated chromagram tail frame is never shorter than num_fft (the reference raises there).

The comparison is test_oracle_parity_seeded's: oracle/paa_oracle.py through assert_parity (contract + tight gate), per clip of
a batch of two clips of different lengths; stereo against the oracle on the downmix, as test_fused_stereo_to_mono does."""
import functools

import numpy as np
import pytest

import paa_oracle as O
from pyaudioanalysis_amd import _ffi
from synth import synth_clip
from test_parity_gpu import assert_parity

pytestmark = pytest.mark.gpu

FRAMES = (29, 42)          # frames of the two clips (plus a few samples that fill no frame)
KINDS = ("i16", "f64", "stereo")
MODES = ("st", "st_deltas", "spectrogram", "chromagram")

# rung -> (fs, window, step, kernel name behind the mode's prefix)
RUNGS = {
    "ct": (16000, 320, 160, "ct_10x16"),
    "tri_a": (44100, 1102, 551, "tri_r19x29x2"),
    "tri_b": (11025, 551, 276, "tri_r29x19"),
    "tri_c": (16000, 256, 128, "tri_4x4x8"),
    "mix": (16000, 200, 100, "mix"),
    "blu_packed": (16000, 346, 174, "blu_512p"),
    "blu_unpacked": (22050, 661, 331, "blu_1024"),
}
CASES = [(r, m, k) for r in RUNGS for m in MODES for k in KINDS]
CASES += [("generic", "spectrogram", k) for k in KINDS]
CASES += [("fast_400", m, "i16") for m in MODES[:2]] + [("fast_800", m, "i16") for m in MODES[:2]]
RUNGS["generic"] = (8000, 100, 50, "generic")
RUNGS["fast_400"] = (16000, 800, 400, "fast_800_w8")
RUNGS["fast_800"] = (16000, 800, 800, "fast_800_s800_w8")


@functools.lru_cache(maxsize=None)
def clips_of(rung):
    """the rung's two stereo clips; a sample type's view of them comes from signal_of"""
    fs, window, step, _ = RUNGS[rung]
    return tuple(synth_clip(4100 + 10 * sorted(RUNGS).index(rung) + i, window + (t - 1) * step + 3 + 4 * i, fs, stereo=True)
                 for i, t in enumerate(FRAMES))


def signal_of(xs, kind):
    """-> (what the plan gets, the mono signal the oracle gets)"""
    if kind == "i16":
        return np.ascontiguousarray(xs[:, 0]), np.ascontiguousarray(xs[:, 0])
    mono = O.stereo_to_mono(xs)
    return (xs, mono) if kind == "stereo" else (mono, mono)


@functools.lru_cache(maxsize=None)
def reference(rung, mode, mono_kind, clip):
    """the oracle's rows of one clip (full-length frames only: a plan leaves the truncated chromagram tail to its caller);
    float64 and stereo plans share the downmix's"""
    fs, window, step, _ = RUNGS[rung]
    mono = signal_of(clips_of(rung)[clip], mono_kind)[1]
    if mode in ("st", "st_deltas"):
        ref = O.feature_extraction(mono, fs, window, step, mode == "st_deltas")[0]
    else:
        rows = (O.spectrogram if mode == "spectrogram" else O.chromagram)(mono, fs, window, step)[0]
        stop = len(mono) - window + 1 if mode == "spectrogram" else len(mono) - step
        full = sum(1 for p in range(window, stop, step) if p + window <= len(mono))
        assert full >= FRAMES[clip] - 3
        ref = np.ascontiguousarray(rows[:full].T)
    ref.setflags(write=False)
    return ref


def run_plan(rung, mode, kind):
    """-> (kernel name, [rows of clip 0, rows of clip 1]) of one plan execution; spectrogram / chromagram rows transposed to
    [bin][frame] like the feature matrix"""
    fs, window, step, _ = RUNGS[rung]
    sigs = [signal_of(xs, kind)[0] for xs in clips_of(rung)]
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in sigs]))).astype(np.int64)
    plan = _ffi.Plan(offsets, fs, window, step, deltas=(mode == "st_deltas"), sample_kind=KINDS.index(kind),
                     mode=max(0, MODES.index(mode) - 1))
    d_in = _ffi.DeviceBuffer.from_host(np.concatenate(sigs))
    d_out = _ffi.DeviceBuffer.from_host(np.zeros(plan.out_doubles))
    try:
        plan.execute(d_in, d_out)
        out = d_out.to_host(np.float64, plan.out_doubles)
        starts = plan.out_offsets()
        name = plan.kernel_name
        width = plan.F
    finally:
        plan.destroy()
        d_in.free()
        d_out.free()
    res = []
    for c in range(2):
        cols = reference(rung, mode, "i16" if kind == "i16" else "f64", c).shape[1]
        slab = out[starts[c]:starts[c] + width * cols]
        res.append(slab.reshape(width, cols).copy() if mode.startswith("st") else np.ascontiguousarray(slab.reshape(cols, width).T))
    return name, res


@pytest.mark.parametrize("rung,mode,kind", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_every_launcher_rung_stores_the_right_rows(gpu_lib, rung, mode, kind):
    fs, window, step, suffix = RUNGS[rung]
    name, res = run_plan(rung, mode, kind)
    assert name == ("st_" if mode.startswith("st") else mode + "_") + suffix          # the family, the shape and the mode's rung
    for c, got in enumerate(res):
        mono_kind = "i16" if kind == "i16" else "f64"
        ref = reference(rung, mode, mono_kind, c)
        what = "%s %s %s clip %d" % (rung, mode, kind, c)
        if mode.startswith("st"):
            assert_parity(got, ref, what, sig=(signal_of(clips_of(rung)[c], kind)[1], fs, window, step))
        else:
            assert_parity(got, ref, what)


def test_lds_attribute_survives_reinitialisation(gpu_lib):
    """The 800/400 kernel runs eight waves on more than 64 KB of LDS, so its launch depends on the raised
    MaxDynamicSharedMemorySize attribute; the launcher's cache of that attribute must not outlive paa_shutdown."""
    first = run_plan("fast_400", "st_deltas", "i16")
    gpu_lib.paa_shutdown()
    _ffi.init(0)
    second = run_plan("fast_400", "st_deltas", "i16")
    assert first[0] == second[0] == "st_fast_800_w8"
    for a, b in zip(first[1], second[1]):
        assert a.tobytes() == b.tobytes()
