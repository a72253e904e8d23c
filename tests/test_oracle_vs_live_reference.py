"""The oracle against outputs of the UNMODIFIED reference on seeded random shapes the other goldens do not cover (those pin
fixed files; this sweeps sampling rates, windows, steps and clip lengths).  CPU only.  What the reference returned (or the type
of what it raised) for every case is stored in tests/golden/live_reference_sweep.npz, written by
`python oracle/make_golden.py --live` from the cases below."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import paa_oracle as O           # noqa: E402
from synth import synth_clip     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "live_reference_sweep.npz")

CHROMA_TAIL_CASES = [(16000, 800, 400, 800 + 400 * 7 + 150), (16000, 800, 400, 800 + 400 * 7 + 390), (16000, 800, 300, 4000),
                     (44100, 44100, 17000, 282240), (44100, 44100, 17000, 276574), (22050, 1103, 441, 9000)]


def feature_case_key(seed, fs, window, step, n):
    return "fe_%d_%d_%d_%d_%d" % (seed, fs, window, step, n)


def chroma_case_key(fs, window, step, n):
    return "chroma_%d_%d_%d_%d" % (fs, window, step, n)


def mid_term_window(window, step):
    return 3 * step + window, 2 * step                       # a few short-term frames per mid-term window


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _case(key, x):
    """The stored outputs of one case; the clip synthesised here must be the one the reference was given."""
    g = {k[len(key) + 2:]: v for k, v in _golden().items() if k.startswith(key + "__")}
    assert g, "%s has no case %s: re-run oracle/make_golden.py --live" % (GOLDEN, key)
    assert str(g["input_sha256"]) == hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest(), key
    return g


def _raises_like(name, fn, *args):
    """fn raises what the reference raised: an exception of type `name` (or of a subclass of it)."""
    with pytest.raises(Exception) as info:
        fn(*args)
    assert str(name) in [c.__name__ for c in type(info.value).__mro__], (name, info.value)


def _cases():
    rng = np.random.default_rng(20260921)
    cases = []
    for k in range(10):
        fs = int(rng.choice([8000, 11025, 16000, 22050, 44100]))
        window = int(rng.integers(int(0.010 * fs), int(0.060 * fs)))
        step = int(rng.integers(max(1, window // 4), window + 1))
        n = int(rng.integers(window, 12 * window))
        cases.append((k, fs, window, step, n))
    cases += [(100, 16000, 800, 400, 800), (101, 16000, 800, 800, 2399), (102, 44100, 1102, 441, 6000)]
    return cases


@pytest.mark.parametrize("seed,fs,window,step,n", _cases())
def test_feature_extraction_and_rows_match_the_running_reference(seed, fs, window, step, n):
    x = synth_clip(7000 + seed, n, fs)
    g = _case(feature_case_key(seed, fs, window, step, n), x)
    # (tiny windows at low sampling rates make the reference's own chroma / mel set-up raise: same exception type)
    if "error" in g:
        _raises_like(g["error"], O.feature_extraction, x, fs, window, step)
        return
    ref, ref_names = g["features"], g["names"]
    got, names = O.feature_extraction(x, fs, window, step)
    assert list(names) == list(ref_names) and got.shape == ref.shape
    assert O.mixed_tolerance_violations(got, ref, rel=1e-9, row_abs=1e-9, abs_floor=1e-12)[0] == 0
    spec = g["specgram"]
    got_spec = O.spectrogram(x, fs, window, step)[0]
    assert got_spec.shape == spec.shape and np.max(np.abs(got_spec - spec)) <= 1e-12 * max(1.0, np.max(np.abs(spec)))
    assert ("mid" in g) == (got.shape[1] >= 4)
    if got.shape[1] >= 4:
        mid_w, mid_s = mid_term_window(window, step)
        rmid, rnames = g["mid"], g["mid_names"]
        gmid, gst, gnames = O.mid_feature_extraction(x, fs, mid_w, mid_s, window, step)
        assert list(gnames) == list(rnames) and gmid.shape == rmid.shape
        assert O.mixed_tolerance_violations(gmid, rmid, rel=1e-9, row_abs=1e-9, abs_floor=1e-12)[0] == 0


@pytest.mark.parametrize("fs,window,step,n", CHROMA_TAIL_CASES)
def test_chromagram_truncated_tail_matches_the_running_reference(fs, window, step, n):
    """chromagram (:324-386) FFTs what is left of a truncated last frame: a tail of at least num_fft samples gives a row, a shorter one fails
    in the reference's scatter (:288-293) -- the oracle returns the same rows or raises the same exception TYPE (round 6: it raised IndexError
    where the reference raises ValueError; found by tests/test_wgs_kernel_gpu.py, whose kernels had it right)."""
    x = synth_clip(7300 + step, n, fs)
    g = _case(chroma_case_key(fs, window, step, n), x)
    if "error" in g:
        _raises_like(g["error"], O.chromagram, x, fs, window, step)
        return
    ref = g["chromagram"]
    got, _, _ = O.chromagram(x, fs, window, step)
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 1e-12
