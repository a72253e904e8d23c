"""The 800-sample int16 kernel (kernels_fast.hpp) on inputs that stress its FP64 arithmetic: digitally silent stretches (the
exact-zero non-DC bins of a constant frame) next to full-scale square waves (the largest bins the int16
range allows, and spread / flux sums whose terms cancel), against the NumPy oracle under the tight gate.  -m gpu."""
import numpy as np
import pytest

import paa_oracle as O
from pyaudioanalysis_amd import ShortTermFeatures, _ffi
from synth import synth_clip
from test_parity_gpu import assert_parity


def edge_clip(seed, fs, seconds):
    """noise, digital silence at 0 and at a nonzero level, full-scale square waves of several periods (none divides the window:
    a line spectrum would leave mel bands of pure round-off, whose MFCCs are ill-conditioned in the reference itself; for the same
    reason the silent stretches sit at moderate levels)"""
    n = int(seconds * fs)
    x = synth_clip(seed, n, fs).astype(np.int16)
    seg = n // 8
    t = np.arange(seg)
    x[1 * seg:2 * seg] = 0                                                              # silence at zero
    x[2 * seg:3 * seg] = np.where((t // 21) % 2 == 0, 32767, -32768)                    # ~381 Hz at 16 kHz, full scale
    x[3 * seg:4 * seg] = -1234                                                          # silence off zero
    x[4 * seg:5 * seg] = np.where((t // 397) % 2 == 0, 32767, -32768)                   # period of about one window
    x[6 * seg:7 * seg] = np.where((t // 3) % 2 == 0, 32767, -32768)                     # near-Nyquist square wave
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("fs,step", [(16000, 400), (16000, 800), (22050, 400)])
@pytest.mark.parametrize("deltas", [False, True])
def test_fast800_silence_and_square_waves(gpu_lib, fs, step, deltas):
    x = edge_clip(17 + step, fs, 4.0)
    plan = _ffi.Plan(np.array([0, x.size], dtype=np.int64), fs, 800, step, deltas=deltas)
    name = plan.kernel_name
    plan.destroy()
    assert "fast" in name, name
    ref, _ = O.feature_extraction(x, fs, 800, step, deltas)
    got, _ = ShortTermFeatures.feature_extraction(x, fs, 800, step, deltas)
    assert_parity(got, ref, "edges 800/%d@%d deltas=%s" % (step, fs, deltas), sig=(x, fs, 800, step))
    # the clip holds digitally silent frames (assert_parity holds their MFCCs to the analytic vector of the exact-zero spectrum)
    frames = (x.size - 800) // step + 1
    silent = np.array([np.all(x[s:s + 800] == x[s]) for s in np.arange(frames) * step])
    assert silent.sum() >= 4
