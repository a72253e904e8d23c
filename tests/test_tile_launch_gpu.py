"""The launch paths the kernel families share (csrc/family_launch.hpp: TileArgs / tile_launch for the one-wave families, WgArgs /
wg_launch for the workgroup-wide ones, with_sample_type): every rung of every family's ladder -- family x mode x sample type --
is reached through a device-resident plan and stores the right rows, and the raised LDS attribute is set again after
paa_shutdown -> paa_init.  -m gpu.

One plan per rung, at the smallest window its family takes (read off the *_select functions): 800/400 and 800/800 int16 for
fast; 320 for ct; 1102, 551 and 256 for the three tri units; 200 for mix (100 = 2^2 5^2 complex points, no register
family); 346 = 2 x 173 for the packed and 661 for the unpacked Bluestein kernel; 100 for generic (fewer than 64 bins: neither
mix nor blu).  The reference itself has no features and no chromagram for a window that small (its chroma table needs about
99 bins), and from 64 bins on mix or blu take every window up to the 8192-point convolution, so generic runs its
spectrogram rung only -- its ladder has one kernel per sample type and no mode rung.  Steps are at least half a window, so
that a truncated chromagram tail frame is never shorter than num_fft (the reference raises there).

The workgroup-wide rungs (WG_RUNGS) run two clips of 5 and 8 frames -- the odd count leaves the task list of the r0 = 6 split
an unpaired frame, the even one gives it pairs -- at a step of half a window, rounded up: both shapes of wgr; the five of wgs
(the two 12 x q ones in st_deltas / int16 only: their ladder is the 6 x q shapes', and a frame costs the oracle 48 000
points); kernels_wg.hpp's whole-transform kernel at 512 threads (9009 = 7 x 9 x 11 x 13 points: radices above 8) and at 768
(spectrogram rung only; 6174 samples = 3087 = 3^2 7^3 points, the smallest window this kernel runs at 768 threads: 12 000 samples
= 6000 points take a radix-16 pass, i.e. 512 threads, and so do 6144; below 6142 samples kernels_mix.hpp has every smooth length),
its split kernel (11 025 points = 3 x 3675) and the passes through HBM (9001, prime); r0 and the thread count are read back
from wg_layout (paa_debug_wg_plan).

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

# the workgroup-wide families (+ the passes through HBM); threads of kernels_wg.hpp's spectrum kernel where it is the rung
WG_FRAMES = (5, 8)
WG_RUNGS = {
    "wgr_10x20x20": (8000, 8000, 4000, "wgr_10x20x20"),
    "wgr_20x20x20": (16000, 16000, 8000, "wgr_20x20x20"),
    "wgs_6x3675": (22050, 22050, 11025, "wgs_6x3675"),
    "wgs_6x4000": (24000, 24000, 12000, "wgs_6x4000"),
    "wgs_8x4000": (32000, 32000, 16000, "wgs_8x4000"),
    "wg_lds_512": (16000, 9009, 4505, "wg_lds_fft"),
    "wg_split": (44100, 11025, 5513, "wg_split_fft"),
    "hbm": (16000, 9001, 4501, "big_window_hbm_passes"),
}
CASES += [(r, m, k) for r in WG_RUNGS for m in MODES for k in KINDS]
WG_RUNGS["wgs_12x3675"] = (44100, 44100, 22050, "wgs_12x3675")
WG_RUNGS["wgs_12x4000"] = (48000, 48000, 24000, "wgs_12x4000")
WG_RUNGS["wg_lds_768"] = (16000, 6174, 3087, "wg_lds_fft")
CASES += [("wgs_12x3675", "st_deltas", "i16"), ("wgs_12x4000", "st_deltas", "i16")]
CASES += [("wg_lds_768", "spectrogram", k) for k in KINDS]
WG_LAYOUT = {"wg_lds_512": (0, 512), "wg_lds_768": (0, 768), "wg_split": (3, None)}      # rung -> (r0, threads) of wg_layout
ALL_RUNGS = dict(RUNGS, **WG_RUNGS)


def frames_of(rung):
    return WG_FRAMES if rung in WG_RUNGS else FRAMES


@functools.lru_cache(maxsize=None)
def clips_of(rung):
    """the rung's two stereo clips; a sample type's view of them comes from signal_of"""
    fs, window, step, _ = ALL_RUNGS[rung]
    seed = 4300 + 10 * sorted(WG_RUNGS).index(rung) if rung in WG_RUNGS else 4100 + 10 * sorted(RUNGS).index(rung)
    return tuple(synth_clip(seed + i, window + (t - 1) * step + 3 + 4 * i, fs, stereo=True)
                 for i, t in enumerate(frames_of(rung)))


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
    fs, window, step, _ = ALL_RUNGS[rung]
    mono = signal_of(clips_of(rung)[clip], mono_kind)[1]
    if mode in ("st", "st_deltas"):
        ref = O.feature_extraction(mono, fs, window, step, mode == "st_deltas")[0]
    else:
        rows = (O.spectrogram if mode == "spectrogram" else O.chromagram)(mono, fs, window, step)[0]
        stop = len(mono) - window + 1 if mode == "spectrogram" else len(mono) - step
        full = sum(1 for p in range(window, stop, step) if p + window <= len(mono))
        assert full >= frames_of(rung)[clip] - 3
        ref = np.ascontiguousarray(rows[:full].T)
    ref.setflags(write=False)
    return ref


def run_plan(rung, mode, kind):
    """-> (kernel name, [rows of clip 0, rows of clip 1]) of one plan execution; spectrogram / chromagram rows transposed to
    [bin][frame] like the feature matrix"""
    fs, window, step, _ = ALL_RUNGS[rung]
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
    fs, window, step, suffix = ALL_RUNGS[rung]
    name, res = run_plan(rung, mode, kind)
    if suffix == "big_window_hbm_passes":
        assert name == suffix          # (one name for every mode)
    else:
        assert name == ("st_" if mode.startswith("st") else mode + "_") + suffix          # the family, the shape and the mode's rung
    if rung in WG_LAYOUT:          # kernels_wg.hpp: which of its spectrum kernels the name stands for
        info = np.zeros(48, dtype=np.int32)
        assert gpu_lib.paa_debug_wg_plan(window, info.ctypes.data_as(_ffi.c_i32p), None, 0) == 1
        r0, threads = WG_LAYOUT[rung]
        assert int(info[3]) == r0 and threads in (None, int(info[6]))
    for c, got in enumerate(res):
        mono_kind = "i16" if kind == "i16" else "f64"
        ref = reference(rung, mode, mono_kind, c)
        what = "%s %s %s clip %d" % (rung, mode, kind, c)
        if mode.startswith("st"):
            assert_parity(got, ref, what, sig=(signal_of(clips_of(rung)[c], kind)[1], fs, window, step))
        else:
            assert_parity(got, ref, what)


REINIT_RUNGS = ("fast_400", "wgr_20x20x20", "wgs_6x3675")


def test_lds_attribute_survives_reinitialisation(gpu_lib):
    """The 800/400 kernel runs eight waves on more than 64 KB of LDS, and so do the workgroups of wgr and wgs: their launch
    depends on the raised MaxDynamicSharedMemorySize attribute, and the launchers' caches of that attribute must not outlive
    paa_shutdown.  On a machine with one GPU the attribute itself survives in the driver, so this guards the path -- same
    kernels, same bits after the re-initialisation -- and does not prove the case of another device."""
    first = [run_plan(r, "st_deltas", "i16") for r in REINIT_RUNGS]
    gpu_lib.paa_shutdown()
    _ffi.init(0)
    second = [run_plan(r, "st_deltas", "i16") for r in REINIT_RUNGS]
    assert [f[0] for f in first] == [s[0] for s in second] == ["st_fast_800_w8", "st_wgr_20x20x20", "st_wgs_6x3675"]
    for f, s in zip(first, second):
        for a, b in zip(f[1], s[1]):
            assert a.tobytes() == b.tobytes()
