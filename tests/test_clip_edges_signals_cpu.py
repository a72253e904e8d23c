"""The signals of tests/test_clip_edges_families_gpu.py, without a device: every one stays inside assert_parity's default
ill-conditioning budget (checks.IllInfo.budget_ok: flagged frames that are not digital silence, at most 1e-3 of the frames),
so the GPU tests rely on no allowance of their own; and the rail clips are what they claim to be."""
import numpy as np
import pytest

from checks import ill_info
from test_clip_edges_families_gpu import CASES, CHUNK, ON_MEAN, SHAPES, loud_last_chunk, mirrored_clip, rail_clip, views


@pytest.mark.parametrize("rung,kind", [c for c in CASES if c[0] != "generic"], ids=["%s-%s" % c for c in CASES if c[0] != "generic"])
def test_rail_clips_stay_inside_the_default_budget(rung, kind):
    fs, window, step, _, _ = SHAPES[rung]
    for mirrored in (False, True):
        mono = views(rail_clip(rung, mirrored), kind)[1]
        info = ill_info(mono, fs, window, step)
        assert info.budget_ok(), (rung, kind, mirrored, info.counts())
        assert not info.silent.any() and len(info.mask) >= 8


def test_rail_clips_sit_near_a_rail():
    for rung in SHAPES:
        x = rail_clip(rung, False)
        assert set(np.unique(x)) == {-32768, 32767} and np.array_equal(rail_clip(rung, True), -1 - x)
        for c in range(2):
            assert 0.78 < np.mean(x[:, c] == -32768) < 0.92
            assert -27000 < x[:, c].mean() < -19000          # x - nearbyint(mean) reaches 55000 on the other rail
            runs = np.diff(np.flatnonzero(np.diff(x[:, c].astype(np.int32))))
            assert len(set(runs)) > 10                      # random dwell times


@pytest.mark.parametrize("rung,kind", ON_MEAN, ids=["%s-%s" % c for c in ON_MEAN])
def test_mirrored_clips_stay_inside_the_default_budget(rung, kind):
    fs, window, step, _, _ = SHAPES[rung]
    mono = views(mirrored_clip(rung), kind)[1]
    assert ill_info(mono, fs, window, step).budget_ok()


def test_inline_fold_clips_stay_inside_the_default_budget():
    for seed, chunks in ((3401, 257), (3402, 193)):
        x = loud_last_chunk(seed, chunks)
        assert len(x) == chunks * CHUNK - 100 and -(-len(x) // CHUNK) == chunks
        a = (chunks - 1) * CHUNK
        assert np.abs(x[:a]).max() < 300 and np.abs(x[a:]).max() > 20000 and x[a:].mean() > 6000 and abs(x[:a].mean()) < 1
        info = ill_info(x, 16000, 320, 320)
        assert info.budget_ok() and not info.silent.any(), info.counts()
