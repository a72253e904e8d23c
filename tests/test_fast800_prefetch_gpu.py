"""The 800-sample int16 kernel (kernels_fast.hpp, steps 400 and 800) stages a quad's samples by one of two paths: from
registers that a 16-byte vector fetch filled earlier (the quad's first sample is 16-byte aligned in the packed buffer and the
clip holds a whole quad, RAW_N = 2000 / 3200 samples, from there), or sample by sample with zero fill.  The two-waves-per-SIMD
instances issue that fetch one quad ahead, behind pass 2 of the quad before, so `pre_ok` and the registers are decided in one
iteration and used in the next.  What this file pins: THE OUTPUT OF A CLIP DOES NOT DEPEND ON WHICH PATH STAGED IT OR ON WHEN
THE FETCH WAS ISSUED.  A clip's alignment is set by what lies before it in a batch (a first clip of 800 + r samples puts the
second at residue r of 8 samples: r = 0 and 8 fetch, every other r falls back everywhere), its last quad's path by its length.
Every comparison is np.array_equal on the uint64 views of the doubles: both paths put the same int16 samples into the same
LDS slots and nothing downstream knows which one ran; no golden is needed.  One case per instance also goes to the NumPy
oracle, so that "equal" cannot mean "equally wrong".  The comparisons already held on the build that fetched at the staging
point (they follow from the tiling invariance the suite asserts elsewhere), so a failure here is a fault of the path, not of
the record.  -m gpu."""
import numpy as np
import pytest

import paa_oracle as O
from pyaudioanalysis_amd import ShortTermFeatures, _ffi
from test_parity_gpu import assert_parity

WINDOW = 800
COMBOS = [(fs, step, deltas) for fs in (16000, 22050) for step in (400, 800) for deltas in (False, True)]
IDS = ["%d_%d_%s" % (fs, step, "d" if deltas else "n") for fs, step, deltas in COMBOS]
POOL = np.random.default_rng(20261111).integers(-12000, 12001, size=70001).astype(np.int16)


def samples(frames, step):
    return WINDOW + (frames - 1) * step


def noise(n, shift):
    """n samples of the pool from `shift` on, repeated end to end where n is longer (its length is no multiple of the steps)."""
    return np.ascontiguousarray(np.resize(np.roll(POOL, -shift), n))


def bits(m):
    return np.ascontiguousarray(m).view(np.uint64)


def alone(x, fs, step, deltas):
    """The clip in a buffer of its own: 16-byte aligned, so every quad with RAW_N samples left is fetched."""
    out, _ = ShortTermFeatures.feature_extraction(x, fs, WINDOW, step, deltas)
    return out


def at_residue(x, r, fs, step, deltas):
    """The clip as the second of a two-clip plan whose first clip has 800 + r samples (one frame)."""
    res, _ = ShortTermFeatures.feature_extraction_batch([noise(WINDOW + r, 4000 + 13 * r), x], fs, WINDOW, step, deltas)
    assert res[0].shape[1] == 1
    return res[1]


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64 == want.dtype, what
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), (what, int((g != w).sum()), np.argwhere(g != w)[:6].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("fs,step,deltas", COMBOS, ids=IDS)
def test_the_instances_are_the_two_wave_fast800_kernels(gpu_lib, fs, step, deltas):
    plan = _ffi.Plan(np.array([0, samples(9, step)], dtype=np.int64), fs, WINDOW, step, deltas=deltas)
    name = plan.kernel_name
    plan.destroy()
    assert "fast_800" in name, name


@pytest.mark.gpu
@pytest.mark.parametrize("fs,step,deltas", COMBOS, ids=IDS)
def test_alignment_sweep(gpu_lib, fs, step, deltas):
    """Nine frames (three quads) behind a first clip of 800 + r samples, r = 0 .. 8: one matrix, the clip's own."""
    x = noise(samples(9, step), 101)
    want = alone(x, fs, step, deltas)
    assert want.shape == (68 if deltas else 34, 9)
    for r in range(9):
        assert_same(at_residue(x, r, fs, step, deltas), want, "residue %d" % r)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,step,deltas", COMBOS, ids=IDS)
def test_length_boundary_of_the_fetch(gpu_lib, fs, step, deltas):
    """pre_ok needs c.n - base >= RAW_N.  The third quad starts at sample 4 * step * 2: with exactly RAW_N samples left it is
    fetched, with one fewer it falls back, and so does a last quad of one frame (800 samples left, and 399 / 799 more than
    that).  Aligned, the earlier quads are fetched; at residue 3 nothing is."""
    raw_n = 3 * step + WINDOW
    third = 8 * step
    lengths = (third + raw_n, third + raw_n - 1, third + WINDOW, third + WINDOW + step - 1)
    assert lengths == ((5200, 5199, 4000, 4399) if step == 400 else (9600, 9599, 7200, 7999))
    for n in lengths:
        x = noise(n, 7 * (n % 1000))
        got = alone(x, fs, step, deltas)
        assert got.shape[1] == (n - WINDOW) // step + 1 and 9 <= got.shape[1] <= 12
        assert_same(got, at_residue(x, 3, fs, step, deltas), "n = %d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,step,deltas", COMBOS, ids=IDS)
def test_runs_of_one_two_and_many_quads(gpu_lib, fs, step, deltas):
    """One frame and four (a single quad: no next fetch), five (a second quad that is the last), and a clip of several runs
    (48 frames without deltas, 150 with: runs that begin on halo frames, so a first fetch at a quad that is not the run's
    first stored frame), each aligned and at residue 3; the multi-run clip also at residue 0 of a batch."""
    for frames in (1, 4, 5, 150 if deltas else 48):
        x = noise(samples(frames, step), 997 * frames)
        want = at_residue(x, 3, fs, step, deltas)             # the fallback path everywhere
        assert want.shape[1] == frames
        assert_same(alone(x, fs, step, deltas), want, "%d frames alone" % frames)
        if frames > 5:
            assert_same(at_residue(x, 0, fs, step, deltas), want, "%d frames at residue 0" % frames)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,step,deltas", COMBOS, ids=IDS)
def test_a_fetched_clip_against_the_oracle(gpu_lib, fs, step, deltas):
    """Twelve frames, three quads, every one of them fetched (the third has exactly RAW_N samples)."""
    x = noise(8 * step + 3 * step + WINDOW, 31337)
    ref, _ = O.feature_extraction(x, fs, WINDOW, step, deltas)
    got = alone(x, fs, step, deltas)
    assert got.shape[1] == 12
    assert_parity(got, ref, "prefetch 800/%d@%d deltas=%s" % (step, fs, deltas), sig=(x, fs, WINDOW, step))
