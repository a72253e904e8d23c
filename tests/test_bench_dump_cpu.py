"""bench.py --dump-outputs: the helper that reads a step's result back (bench.dump_outputs), on host arrays laid out like the
device buffers -- clips back to back, a [rows][T_c] matrix each.  A dump that fits holds every frame; a larger one a seeded
sample of frames that is the same from run to run and stays under the limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _job(rows, frames, gap=0):
    """flat buffer with `gap` unused doubles between the slabs, the per-clip matrices, the slab offsets"""
    rng = np.random.default_rng(7)
    mats = [rng.standard_normal((rows, t)) for t in frames]
    offsets, pos, parts = [], 0, []
    for m in mats:
        offsets.append(pos)
        parts += [m.reshape(-1), np.full(gap, np.nan)]
        pos += m.size + gap
    return np.concatenate(parts), mats, np.array(offsets, dtype=np.int64)


def _fetch(buf, calls=None):
    def fetch(off, cnt):
        assert 0 <= off and off + cnt <= buf.size
        if calls is not None:
            calls.append(cnt)
        return buf[off:off + cnt].copy()
    return fetch


def test_a_dump_that_fits_holds_every_frame_in_clip_order(tmp_path):
    frames = [5, 1, 12, 3]
    buf, mats, offsets = _job(34, frames, gap=3)
    info = bench.dump_outputs(str(tmp_path), _fetch(buf), 34, frames, offsets)
    got = np.load(tmp_path / "features.npy")
    idx = np.load(tmp_path / "frame_index.npy")
    assert got.dtype == np.float64 and idx.dtype == np.float64
    assert np.array_equal(got, np.concatenate(mats, axis=1))
    assert np.array_equal(idx, np.arange(sum(frames)))
    assert info["frames_dumped"] == sum(frames) and not info["sampled"]


def test_a_large_dump_is_a_seeded_sample_under_the_limit(tmp_path, monkeypatch):
    rows, frames = 68, [400] * 30 + [2500]
    buf, mats, offsets = _job(rows, frames)
    limit = 64 * 1024
    monkeypatch.setattr(bench, "DUMP_CHUNK_DOUBLES", 3 * rows * 400)      # several copies, one clip larger than a copy
    calls = []
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        info = bench.dump_outputs(str(d), _fetch(buf, calls), rows, frames, offsets, limit=limit)
        assert info["sampled"] and 0 < info["frames_dumped"] < sum(frames)
        assert sum(os.path.getsize(d / n) for n in ("features.npy", "frame_index.npy")) <= limit
    assert max(calls) == rows * 2500 and len(calls) > 2
    a, b = (np.load(d / "features.npy") for d in dirs)
    ia, ib = (np.load(d / "frame_index.npy") for d in dirs)
    assert np.array_equal(a, b) and np.array_equal(ia, ib)
    assert np.all(np.diff(ia) > 0)
    whole = np.concatenate(mats, axis=1)
    assert np.array_equal(a, whole[:, ia.astype(np.int64)])
