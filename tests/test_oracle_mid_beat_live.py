"""The oracle's mid-term statistics and beat extraction against the UNMODIFIED reference on designed short-term matrices
(oracle/synth.py designed_matrix): the edges the GPU tests of tests/test_aux_kernels_gpu.py hold the mid_stats_kernel and
beat_kernel to -- negative, zero and long mid-term windows, steps longer than the window, clips of 1..3 frames, frame
counts around the beat kernel's 128-frame tile, histograms of 1 to 2 000 bins and of none.  CPU only.  What the reference
returned (or the type of what it raised) for every case is stored in tests/golden/live_reference_mid_beat.npz, written by
`python oracle/make_golden.py --live` from the cases below; when the reference tree is present the cases also run live."""
import contextlib
import functools
import hashlib
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import load_reference            # noqa: E402
import paa_oracle as O           # noqa: E402
from synth import designed_matrix  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "live_reference_mid_beat.npz")

MID_ROWS = 9                     # one row of every designed kind
MID_FRAMES = (1, 2, 17, 100)
MID_RATIOS = (-7, -1, 0, 1, 2, 63, 64, 65, 200)
BEAT_FRAMES = (1, 2, 3, 127, 128, 129, 257, 700)
BEAT_WINDOWS = (0.05, 0.025, 0.0025, 0.001, 2.0, 3.0, 5.0)
# (mid_window, mid_step, short_window, short_step) as the public entry points get them: banker's rounding of 2.5 and 3.5
# (2 and 4, not 3 and 4), a mid window given in seconds (ratio -1), a ratio of 0 and of 1, a step longer than the window
RATIO_ARGS = ((1400, 1000, 800, 400), (1800, 1400, 800, 400), (0.5, 8000, 800, 400), (400, 400, 800, 400),
              (800, 400, 800, 400), (2000, 6000, 800, 400), (16000, 8000, 800, 400))
RATIO_FRAMES = 60


def mid_step_ratios(ratio, n_frames):
    """1, 3, the ratio itself and a step longer than it; on the long clip 1 and 3 only where the window is short or on the
    64 / 65 boundary (the fixture stays small)."""
    short = n_frames <= 17
    steps = {ratio, ratio + 4} | ({1} if short else set()) | ({3} if short or ratio <= 2 or ratio in (64, 65) else set())
    return sorted(s for s in steps if s >= 1)


def mid_cases():
    out = []
    for T in MID_FRAMES:
        for ratio in MID_RATIOS + (T + 5,):
            for step in mid_step_ratios(ratio, T):
                out.append((T, ratio, step))
    return out


def mid_matrix(T):
    return designed_matrix(900 + T, MID_ROWS, T)


def beat_matrix(T):
    return designed_matrix(500 + T, 19, T, nonfinite=False)


def ratio_matrix():
    return designed_matrix(77, MID_ROWS, RATIO_FRAMES)


def mid_case_key(T, ratio, step):
    return "mid_%d_%d_%d" % (T, ratio, step)


def ratio_case_key(args):
    return "ratio_" + "_".join(repr(a).replace(".", "p") for a in args)


def matrix_key(what, T):
    """Key of the SHA-256 of an input matrix (stored once per matrix, not per case)."""
    return "input_%s_%d__sha256" % (what, T)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the reference, driven on a given short-term matrix -----------------------------------------------------------------
def reference_mid(ref_st, ref_mt, matrix, mid_window, mid_step, short_window, short_step):
    """The reference's mid_feature_extraction loop (MidTermFeatures.py:87-127) on `matrix`: its feature_extraction call is
    replaced by one that returns the matrix (the signal is not looked at)."""
    names = ["f%d" % i for i in range(matrix.shape[0])]
    saved = ref_st.feature_extraction
    ref_st.feature_extraction = lambda *a, **k: (matrix.copy(), list(names))
    try:
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                mid, _, _ = ref_mt.mid_feature_extraction(np.zeros(8), 16000, mid_window, mid_step, short_window, short_step)
    finally:
        ref_st.feature_extraction = saved
    return np.asarray(mid, dtype=np.float64)


def reference_beat(ref_mt, matrix, window):
    import warnings
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref_mt.beat_extraction(matrix, window)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _case(key, what, x):
    """The stored outputs of one case; the matrix made here must be the one the reference was given."""
    g = {k[len(key) + 2:]: v for k, v in _golden().items() if k.startswith(key + "__")}
    assert g, "%s has no case %s: re-run oracle/make_golden.py --live" % (GOLDEN, key)
    assert str(_golden()[matrix_key(what, x.shape[1])]) == sha(x), key
    return g


@functools.lru_cache(maxsize=None)
def _live():
    if not load_reference.reference_available():
        return None
    ref_st, ref_mt, _ = load_reference.load()
    return ref_st, ref_mt


def _raises_like(name, fn, *args):
    with pytest.raises(Exception) as info:
        fn(*args)
    assert str(name) in [c.__name__ for c in type(info.value).__mro__], (name, info.value)


def test_fixture_is_small_and_has_a_kind():
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert str(_golden()["kind"]) == "live_mid_beat"


@pytest.mark.parametrize("T,ratio,step", mid_cases())
def test_mid_statistics_match_the_reference(T, ratio, step):
    x = mid_matrix(T)
    g = _case(mid_case_key(T, ratio, step), "mid", x)
    got = O.mid_statistics(x, ratio, step)
    assert got.shape == g["mid"].shape
    assert np.array_equal(got, g["mid"])           # the same NumPy reductions on the same slices
    if _live():
        assert np.array_equal(got, reference_mid(*_live(), x, ratio, step, 1, 1))


@pytest.mark.parametrize("args", RATIO_ARGS, ids=ratio_case_key)
def test_mid_ratios_match_the_reference(args):
    x = ratio_matrix()
    g = _case(ratio_case_key(args), "ratio", x)
    ratio, step = O.mid_ratios(*args)
    got = O.mid_statistics(x, ratio, step)
    assert got.shape == g["mid"].shape and np.array_equal(got, g["mid"])
    if _live():
        assert np.array_equal(got, reference_mid(*_live(), x, *args))


def test_ratio_cases_reach_the_edges():
    got = [O.mid_ratios(*a) for a in RATIO_ARGS]
    assert got[0] == (2, 2) and got[1] == (4, 4)            # banker's rounding of 2.5 / 3.5 (half-up: 3, 4 and 3, 4)
    assert got[2][0] == -1 and got[3][0] == 0 and got[4][0] == 1
    assert got[5][1] > got[5][0] >= 1


@pytest.mark.parametrize("T", BEAT_FRAMES)
@pytest.mark.parametrize("window", BEAT_WINDOWS)
def test_beat_extraction_matches_the_reference(T, window):
    x = beat_matrix(T)
    g = _case("beat_%d" % T, "beat", x)
    w = BEAT_WINDOWS.index(window)
    if str(g["error"][w]):
        _raises_like(g["error"][w], O.beat_extraction, x, window)
        if _live():
            _raises_like(g["error"][w], reference_beat, _live()[1], x, window)
        return
    bpm, conf = O.beat_extraction(x, window)
    assert bpm == g["bpm"][w]
    assert abs(conf - g["ratio"][w]) <= 1e-12 * abs(g["ratio"][w])
    if _live():
        rb, rc = reference_beat(_live()[1], x, window)
        assert bpm == rb and abs(conf - rc) <= 1e-12 * abs(rc)


def test_beat_cases_reach_the_edges():
    g = _golden()
    assert [str(e) for e in g["beat_700__error"]] == [""] * 6 + ["ValueError"]          # window_size 5.0: no bins
    # the designed rows give the histograms something to count: a non-zero confidence on the longer clips
    assert all(g["beat_%d__ratio" % T][0] > 0 for T in (127, 257, 700))
