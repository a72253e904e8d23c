"""bench.synth_clips: the threaded, chunked synthesis of the bench's input clips gives exactly the samples of
oracle/synth.synth_clip (the timed steps must read the same bytes as before), whatever the chunk size and the worker count."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from synth import synth_clip  # noqa: E402


@pytest.mark.parametrize("n, chunk, workers", [
    (60 * 16000, 1 << 18, None),       # the default chunk, the last one partial
    (10 * 16000, 1000, 4),             # the zeroed 0.5 s span crosses several chunk boundaries
    (10 * 16000, 7919, 1),             # a chunk that divides nothing, one worker
    (8000, 3000, 2),                   # exactly the span: no zeroed run drawn
    (5000, 1 << 18, 3),                # shorter than the span
])
def test_synth_clips_equals_synth_clip(n, chunk, workers):
    seeds = [2, 1002, 2002, 40000]
    got = bench.synth_clips(seeds, n, chunk=chunk, workers=workers)
    for seed, x in zip(seeds, got):
        ref = synth_clip(seed, n, bench.FS)
        assert x.dtype == ref.dtype == np.int16 and x.shape == ref.shape
        assert np.array_equal(x, ref), seed


def test_synth_clips_other_rate():
    got = bench.synth_clips([5], 3 * 8000, fs=8000, chunk=5000)
    assert np.array_equal(got[0], synth_clip(5, 3 * 8000, 8000))
