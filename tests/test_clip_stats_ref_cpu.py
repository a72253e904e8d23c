"""The exact-arithmetic reference of tests/test_clip_stats_gpu.py against the oracle's normalisation (paa_oracle.normalize_clip:
x / 2^15, minus the clip mean, over max|.| + 1e-10; ShortTermFeatures.py:14-19, :567-570): the integer formula gives NumPy's mean
and maximum bit for bit -- every partial sum of either is exact below 2^53.  Plus the argument checks of
paa_debug_plan_clip_norms that need no device."""
import numpy as np
import pytest

import paa_oracle as O
from pyaudioanalysis_amd import _ffi
from synth import synth_clip
from test_clip_stats_gpu import I16, STEREO, counts_of, derived, exact_int


def clips():
    rng = np.random.default_rng(2100)
    yield "synth", I16, synth_clip(2101, 48000, 16000)
    yield "synth stereo", STEREO, synth_clip(2102, 30011, 16000, stereo=True)
    yield "full scale noise", I16, rng.integers(-32768, 32768, 1 << 20).astype(np.int16)
    yield "full scale stereo noise", STEREO, rng.integers(-32768, 32768, (777777, 2)).astype(np.int16)
    yield "near the negative rail", I16, np.where(rng.random(100003) < 0.85, -32768, 32767).astype(np.int16)
    yield "negative rail", I16, np.full(4097, -32768, dtype=np.int16)
    yield "odd stereo total", STEREO, np.tile(np.array([[4, 5]], dtype=np.int16), (1001, 1))
    yield "ripple on an offset", I16, (1000 + rng.integers(-3, 4, 321)).astype(np.int16)


@pytest.mark.parametrize("what,kind,sig", list(clips()), ids=[c[0] for c in clips()])
def test_integer_formula_is_the_oracles_mean_and_maximum(what, kind, sig):
    mono = O.stereo_to_mono(sig) if kind == STEREO else sig
    x = np.double(mono) / (2.0 ** 15)
    mean = x.mean()
    peak = np.abs(x - mean).max()
    c = counts_of(sig, kind)
    ref = exact_int(int(c.sum()), int(c.min()), int(c.max()), len(c), kind, 320)
    assert ref["mean"] == mean
    assert ref["inv"] == 1.0 / (peak + 1e-10)
    y = O.normalize_clip(mono)
    assert np.array_equal(y, (x - ref["mean"]) * 1.0 if peak == 0 else (x - ref["mean"]) / (peak + 1e-10))
    assert np.abs(y).max() == peak / (peak + 1e-10)


def test_derived_constants_restated():
    d = derived(4.5 / 32768.0, 2.0, 320)
    assert (d["mu"], d["m_int"], d["delta_mu"], d["zb"], d["mu_whole"], d["dc_shift"]) == (4.5, 4.0, 0.5, 4.0, 0.0, 320.0)
    d = derived(-5.5 / 32768.0, 2.0, 800)
    assert (d["m_int"], d["delta_mu"], d["zb"], d["mu_whole"], d["dc_shift"]) == (-6.0, 0.5, -6.0, 0.0, 800.0)
    d = derived(-50000.0 / 32768.0, 1.0, 2)
    assert (d["m_int"], d["zb"], d["mu_whole"]) == (-40000.0, -32768.0, 1.0)
    d = derived(50000.5 / 32768.0, 1.0, 2)
    assert (d["m_int"], d["zb"], d["mu_whole"]) == (40000.0, 32767.0, 0.0)


def test_accessor_is_exported_and_judges_its_arguments():
    lib = _ffi.lib()
    assert "paa_debug_plan_clip_norms" in _ffi.EXPORTED_SYMBOLS
    out = np.zeros(20)
    assert lib.paa_debug_plan_clip_norms(None, None, None, 0) == _ffi.ERR_ARG
    assert lib.paa_debug_plan_clip_norms(None, out.ctypes.data, _ffi.as_f64p(out), 20) == _ffi.ERR_ARG
    assert np.all(out == 0.0)
