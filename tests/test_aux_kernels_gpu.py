"""GPU tests of the two kernels that run after the feature matrix -- mid_stats_kernel (mid-term mean / std) and beat_kernel
(MidTermFeatures.beat_extraction) -- in isolation: designed short-term matrices (oracle/synth.py designed_matrix) are uploaded
into the slabs of a plan and the kernels' results are compared with the oracle on the same matrices, whose agreement with the
unmodified reference on these edges is pinned by tests/test_oracle_mid_beat_live.py.  Then the public mid-term entry points at
their argument edges, end to end."""
import numpy as np
import pytest

import paa_oracle as O
from pyaudioanalysis_amd import MidTermFeatures, _ffi
from synth import designed_matrix
from test_oracle_mid_beat_live import BEAT_FRAMES, MID_RATIOS, mid_step_ratios
from test_parity_gpu import assert_parity

pytestmark = pytest.mark.gpu

WINDOW, STEP, FS = 800, 400, 16000
MID_CLIP_FRAMES = (1, 2, 17, 64, 65, 1003)
BEAT_WINDOWS = (0.05, 0.025, 0.0025, 0.001, 2.0, 3.0)        # 0.0025 s: > 64 KB of LDS; 0.001 s: just under 160 KB


class DesignedPlan:
    """A plan over clips of the given frame counts whose short-term slabs hold designed matrices instead of features."""

    def __init__(self, frames, n_rows, seed, nonfinite=True):
        lens = [WINDOW + (T - 1) * STEP for T in frames]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.plan = _ffi.Plan(offsets, FS, WINDOW, STEP, deltas=(n_rows == 68))
        assert self.plan.F == n_rows
        self.frames = list(frames)
        self.mats = [designed_matrix(seed + i, n_rows, T, nonfinite) for i, T in enumerate(frames)]
        flat = np.zeros(self.plan.out_doubles)
        ends = list(self.plan.out_offsets()[1:]) + [self.plan.out_doubles]
        for o, end, m in zip(self.plan.out_offsets(), ends, self.mats):
            assert int(end) - int(o) == m.size
            flat[int(o):int(o) + m.size] = m.ravel()
        self.d_st = _ffi.DeviceBuffer.from_host(flat)

    def mid(self, ratio, step):
        n = self.plan.mid_doubles(step)
        d_mid = _ffi.DeviceBuffer(n * 8)
        self.plan.mid_execute(self.d_st, ratio, step, d_mid)
        flat = d_mid.to_host(np.float64, n)
        out, pos = [], 0
        for T in self.frames:
            M = -(-T // step)
            out.append(flat[pos:pos + 2 * self.plan.F * M].reshape(2 * self.plan.F, M))
            pos += 2 * self.plan.F * M
        assert pos == n
        return out

    def beat(self, window):
        d_beat = _ffi.DeviceBuffer(16 * len(self.frames))
        self.plan.beat_execute(self.d_st, window, d_beat)
        return d_beat.to_host(np.float64, 2 * len(self.frames)).reshape(-1, 2)

    def destroy(self):
        self.plan.destroy()


def assert_mid_matches(got, x, ratio, step, what):
    """Windows holding NaN / +-inf: exactly the oracle's nan_to_num values.  Empty windows: 0.  The rest: means within 1e-12
    relative plus 1e-12 of the row's largest finite |value|; standard deviations through their squares (a 1e6 offset with a
    1e-6 spread leaves any two summation orders a mean apart by ~1e-10, i.e. the variances by ~1e-20)."""
    ref = O.mid_statistics(x, ratio, step)
    F, T = x.shape
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    lims = [slice(b, min(b + ratio, T)).indices(T)[:2] for b in range(0, T, step)]
    b = np.array([lo for lo, _ in lims])
    e = np.maximum(np.array([hi for _, hi in lims]), b)
    nf = np.concatenate([np.zeros((F, 1)), np.cumsum(~np.isfinite(x), axis=1)], axis=1)
    nonfinite = np.tile((nf[:, e] - nf[:, b]) > 0, (2, 1))
    assert np.array_equal(got[nonfinite], ref[nonfinite]), what
    empty = np.tile(e == b, (2 * F, 1))
    assert not np.any(got[empty]), what
    scale = np.max(np.where(np.isfinite(x), np.abs(x), 0.0), axis=1)[:, None]
    ok = ~nonfinite & ~empty
    gm, rm = got[:F], ref[:F]
    bad_mean = (np.abs(gm - rm) > 1e-12 * np.abs(rm) + 1e-12 * scale) & ok[:F]
    gs, rs = got[F:], ref[F:]
    bad_std = (np.abs(gs * gs - rs * rs) > 1e-12 * rs * rs + (1e-14 * scale) ** 2) & ok[F:]
    bad = np.concatenate([bad_mean, bad_std])
    if bad.any():
        idx = np.argwhere(bad)[:6]
        raise AssertionError("%s: %d entries differ: %s" % (what, int(bad.sum()), ", ".join(
            "[%d,%d] %.17g vs %.17g" % (i, j, got[i, j], ref[i, j]) for i, j in idx)))


@pytest.fixture(scope="module")
def mid_plans(gpu_lib):
    plans = {F: DesignedPlan(MID_CLIP_FRAMES, F, 3000 + F) for F in (68, 34)}
    yield plans
    for p in plans.values():
        p.destroy()


MID_PAIRS = sorted({(r, s) for r in MID_RATIOS + (max(MID_CLIP_FRAMES) + 5,) for s in mid_step_ratios(r, 17)})


@pytest.mark.parametrize("ratio,step", MID_PAIRS)
def test_mid_stats_kernel_designed_rows(mid_plans, ratio, step):
    """Every (ratio, step ratio) of the oracle pin on one ragged plan (1 to ~1 000 frames, so the grid sized by the longest
    clip idles most blocks of the others): negative ratios (Python's negative slice stop), 0, the 64 / 65 boundary between the
    register path and the loop, windows longer than the clip, steps longer than the window."""
    for F in (68, 34):
        if F == 34 and abs(ratio) not in (1, 7, 64, 65):
            continue
        p = mid_plans[F]
        for T, x, got in zip(p.frames, p.mats, p.mid(ratio, step)):
            assert_mid_matches(got, x, ratio, step, "F=%d T=%d ratio=%d step=%d" % (F, T, ratio, step))


def test_mid_stats_negative_ratio_windows_are_not_empty(mid_plans):
    """ratio = -1: window 0 is frames [0, T - 1) (the reference's row[0:-1]), not an empty window."""
    p = mid_plans[68]
    got = p.mid(-1, 3)
    T, x = p.frames[-1], p.mats[-1]
    assert got[-1][0, 0] != 0.0
    assert abs(got[-1][1, 0] - np.mean(x[1, :T - 1])) <= 1e-12 * abs(np.mean(x[1, :T - 1])) + 1e-12 * np.max(np.abs(x[1]))


def test_mid_stats_step_cache_a_b_a(mid_plans):
    """The per-plan cache of the output offsets (keyed by the step ratio) across steps A, B, A."""
    p = mid_plans[68]
    first = p.mid(10, 3)
    second = p.mid(10, 7)
    third = p.mid(10, 3)
    for T, x, a, b, c in zip(p.frames, p.mats, first, second, third):
        assert_mid_matches(a, x, 10, 3, "A T=%d" % T)
        assert_mid_matches(b, x, 10, 7, "B T=%d" % T)
        assert np.array_equal(a, c)


# ---- public entry points -------------------------------------------------------------------------------------------------
def _clip(seed, n, stereo=False):
    """Sines + noise without digital silence (synth_clip zeroes a 0.5 s span)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    chans = []
    for _ in range(2 if stereo else 1):
        x = sum(rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * rng.uniform(80, 7000) * t + rng.uniform(0, 6)) for _ in range(4))
        chans.append(np.clip(np.round(5000 * x + 800 * rng.standard_normal(n)), -32768, 32767).astype(np.int16))
    return np.stack(chans, axis=1) if stereo else chans[0]


# (mid_window, mid_step, short_window, short_step): ratio -1 (mid window in seconds), ratio 1, a mid window longer than the
# clip, a step larger than the window, banker's rounding of 2.5 and 3.5, the usual 1 s / 1 s
ENTRY_ARGS = [(0.5, 8000, 800, 400), (800, 400, 800, 400), (400000, 8000, 800, 400), (2000, 6000, 800, 400),
              (1400, 1000, 800, 400), (1800, 1400, 800, 400), (16000, 16000, 800, 400)]


@pytest.mark.parametrize("args", ENTRY_ARGS, ids=lambda a: "_".join(str(v) for v in a))
def test_mid_feature_extraction_entry_points_at_argument_edges(gpu_lib, args):
    ratio, step = O.mid_ratios(*args)
    clips = [_clip(41, 3 * FS + 123), _clip(42, FS // 2 + 7), _clip(43, 2 * FS)]
    for kind, sig in (("int16", clips[0]), ("float64", clips[0].astype(np.float64)), ("stereo", _clip(44, 2 * FS, True))):
        mid, st, names = MidTermFeatures.mid_feature_extraction(sig, FS, *args)
        mono = O.stereo_to_mono(sig) if sig.ndim == 2 else sig
        ref_mid, ref_st, ref_names = O.mid_feature_extraction(mono, FS, *args)
        assert names == ref_names
        what = "%s ratio=%d step=%d" % (kind, ratio, step)
        assert_parity(st, ref_st, what + " short", sig=(mono, FS, args[2], args[3]))
        assert_parity(mid, ref_mid, what + " mid", sig=(mono, FS, args[2], args[3]))
    singles = [MidTermFeatures.mid_feature_extraction(c, FS, *args)[0] for c in clips]
    mids, _ = MidTermFeatures.mid_feature_extraction_batch(clips, FS, *args)
    mids2, beats = MidTermFeatures.mid_and_beat_batch(clips, FS, *args, beat_window_seconds=args[3] / FS)
    for c, one in enumerate(singles):
        assert np.array_equal(mids[c], one) and np.array_equal(mids2[c], one), c


# ---- beat ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beat_plans(gpu_lib):
    plans = {F: DesignedPlan(BEAT_FRAMES, F, 5000 + F, nonfinite=False) for F in (68, 34)}
    yield plans
    for p in plans.values():
        p.destroy()


@pytest.mark.parametrize("window", BEAT_WINDOWS)
def test_beat_kernel_designed_rows(beat_plans, window):
    """Constant rows (threshold floor 1e-16), plateaus with exact ties, spikes with gaps longer than max_beat, clips of 1..3
    frames and around the 128-frame LDS tile; histograms of 1 to 2 000 bins (0.0025 s runs the > 64 KB launch).  The
    single-matrix entry against the oracle, the batched entry bit for bit against it."""
    for F, p in beat_plans.items():
        batch = p.beat(window)
        for c, (T, x) in enumerate(zip(p.frames, p.mats)):
            bpm, conf = MidTermFeatures.beat_extraction(x, window)
            rb, rc = O.beat_extraction(x, window)
            what = "F=%d T=%d window=%g" % (F, T, window)
            assert bpm == rb, (what, bpm, rb)
            assert abs(conf - rc) <= 1e-12 * abs(rc), (what, conf, rc)
            assert batch[c, 0] == bpm and batch[c, 1] == conf, what


def test_beat_histogram_without_bins_raises_like_the_reference(beat_plans):
    """window_size >= 4 s: round(2 / window_size) = 0 bins, the reference's argmax of the empty histogram raises ValueError."""
    x = beat_plans[68].mats[-1]
    with pytest.raises(ValueError):
        O.beat_extraction(x, 5.0)
    with pytest.raises(ValueError):
        MidTermFeatures.beat_extraction(x, 5.0)
    with pytest.raises(ValueError):
        beat_plans[68].beat(5.0)
    with pytest.raises(ValueError):
        MidTermFeatures.mid_and_beat_batch([_clip(45, FS)], FS, FS, FS, 800, 400, beat_window_seconds=4.0)


def test_beat_histogram_beyond_the_lds_limit_raises(beat_plans):
    """More than 2 017 bins do not fit the 160 KB of LDS of one workgroup: the documented NotImplementedError."""
    x = beat_plans[68].mats[-1]
    with pytest.raises(NotImplementedError):
        MidTermFeatures.beat_extraction(x, 0.00099)
    with pytest.raises(NotImplementedError):
        beat_plans[34].beat(0.00099)
