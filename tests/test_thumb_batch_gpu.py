"""music_thumbnailing_batch on the GPU: clip i of any batch must EQUAL its own single call -- the similarity matrix of
paa_self_similarity_f64, the filtered matrix and arg-max of paa_dev_thumbnail_filter / paa_thumbnail_f64 bit for bit (NaN
pattern included), the four times of music_thumbnailing -- at any position, beside any other clips, under any chunk_bytes.
Against the reference the gates are those of tests/test_similarity_gpu.py: 1e-9 * m on a filtered matrix from the same
features or matrix, 2e-5 * m through the HIP feature path, positions identical.  -m gpu."""
import glob
import os

import numpy as np
import pytest

import sim_ref
import thumb_batch_cases as cases
from conftest import GOLDEN_DIR, load_golden
from pyaudioanalysis_amd import _ffi, audioSegmentation as aS
from synth import synth_song

pytestmark = pytest.mark.gpu

GRAM_T = (1, 2, 127, 128, 129, 257, 385)
FILTER_SIZES = tuple(p for p in sim_ref.THUMB_SIZES if p[0] <= 319)
BAND = 3.0


def _nan_equal_bits(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert sim_ref.same_bits(a, b), "%s: bits differ (max abs diff %g)" % (what, np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max(initial=0.0))


_single_cache = {}


def _single(lib, S, M, band, l1, l2, key):
    """paa_dev_thumbnail_filter of one matrix: (filtered, (row, column)); one call per distinct input of this module"""
    k = (key, M, band, l1, l2)
    if k not in _single_cache:
        rc, filt, pos, guard = sim_ref.dev_thumbnail_filter(lib, S, M, band, l1, l2)
        assert rc == 0 and sim_ref.untouched(guard)
        _single_cache[k] = (filt, pos)
    return _single_cache[k]


def _check_against_single(lib, mats, keys, M, band, l1=0, l2=1, **kw):
    """one batch of matrices against the single call per clip: filtered bits, arg-max, and the walk on the returned matrix"""
    out = aS.thumbnail_filter_batch(mats, M, band, l1, l2, **kw)
    assert len(out) == len(mats)
    for c, (S, key) in enumerate(zip(mats, keys)):
        filt, pos, bounds = out[c]
        want_filt, want_pos = _single(lib, S, M, band, l1, l2, key)
        _nan_equal_bits(filt, want_filt, "clip %d (%s)" % (c, key))
        assert pos == want_pos, (c, key, pos, want_pos)
        assert bounds == aS._grow_thumbnail(filt, pos[0], pos[1], M), (c, key)
    return out


# ---- stage 1 and 2: ragged Gram batch ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gram_inputs(gpu_lib):
    """feature matrices of the ragged batch and their single-call matrices, computed once"""
    out = {}
    for n_dims in (68, 5):
        mats = [sim_ref.seeded_features(n_dims, t) for t in GRAM_T]
        out[n_dims] = (mats, [aS.self_similarity_matrix(f) for f in mats])
    return out


@pytest.mark.parametrize("n_dims", [68, 5])
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_ragged_gram_batch_equals_the_single_calls(gram_inputs, n_dims, order):
    mats, singles = gram_inputs[n_dims]
    idx = list(range(len(mats)))[::-1] if order == "reversed" else list(range(len(mats)))
    sims = aS.self_similarity_batch([mats[i] for i in idx])
    for c, i in enumerate(idx):
        S = sims[c]
        assert S.shape == (GRAM_T[i], GRAM_T[i])
        _nan_equal_bits(S, singles[i], "T = %d at position %d" % (GRAM_T[i], c))
        assert np.all(np.diag(S) == 1.0)
        assert sim_ref.same_bits(S, S.T), "T = %d: not bitwise symmetric" % GRAM_T[i]


# ---- stage 3 and 4: filter batch -----------------------------------------------------------------------------------------------------
def _reference_check(S, M, band, filt, pos):
    ref = sim_ref.thumbnail_filter(S, M, band)
    d = np.abs(np.asarray(filt, dtype=sim_ref.LD) - ref)
    assert float(d.max()) <= 1e-9 * M, (S.shape[0], M, float(d.max()))
    ref_pos, margin = sim_ref.argmax_margin(np.asarray(ref, dtype=np.float64))
    if margin > 2e-9 * M:                      # the maximum stands clear of what the gate allows on both cells
        assert pos == ref_pos, (S.shape[0], M, pos, ref_pos)


@pytest.mark.parametrize("M", sorted({m for _, m in FILTER_SIZES}))
def test_filter_batch_of_every_size(gpu_lib, M):
    """every n of THUMB_SIZES (n <= 319) that admits this filter length, in ONE batch"""
    ns = [n for n, _ in FILTER_SIZES if n >= M]
    mats = [cases.symmetric_matrix(n, 100 + n) for n in ns]
    out = _check_against_single(gpu_lib, mats, ["sym%d" % n for n in ns], M, BAND)
    for S, (filt, pos, _) in zip(mats, out):
        _reference_check(S, M, BAND, filt, pos)


def test_filter_batch_at_the_run_seams(gpu_lib):
    """M = 32 over n = 32 (R = 1), 33, 63 (R = 32: one run), 64 (R = 33), 65, 287 (R = 256: one x block exactly)"""
    ns = (32, 33, 63, 64, 65, 287)
    mats = [cases.symmetric_matrix(n, 200 + n) for n in ns]
    out = _check_against_single(gpu_lib, mats, ["seam%d" % n for n in ns], 32, BAND)
    for S, (filt, pos, _) in zip(mats, out):
        _reference_check(S, 32, BAND, filt, pos)
    assert out[0][0].shape == (1, 1) and out[0][1] == (0, 0) and out[0][2] == (0, 0, 0, 0)


# ---- exact and special matrices among ordinary clips ---------------------------------------------------------------------------------
def test_special_matrices_inside_one_batch(gpu_lib):
    M, band, n = 7, 10.0, 200
    special = {"tied": sim_ref.tied_matrix(n), "dyadic": sim_ref.dyadic_matrix(130, 5)}
    special.update({"degenerate_" + k: v for k, v in sim_ref.degenerate_matrices(150, band).items()})
    special.update({"nan_" + k: v for k, v in sim_ref.nan_matrices(n, 11).items()})
    names, mats = [], []
    for k, (name, S) in enumerate(special.items()):             # an ordinary clip before every special one, and one at the end
        names += ["sym%d" % (90 + 13 * k), name]
        mats += [cases.symmetric_matrix(90 + 13 * k, 300 + k), S]
    names.append("sym77")
    mats.append(cases.symmetric_matrix(77, 399))
    out = _check_against_single(gpu_lib, mats, names, M, band)
    got = dict(zip(names, out))
    for name, (filt, pos, _) in got.items():                     # numpy's arg-max: first maximum in row-major order, NaN first
        assert pos == sim_ref.argmax_margin(filt)[0], name
    count, x_blocks, y_blocks, _ = sim_ref.tie_spread(got["tied"][0])
    assert count > 1 and y_blocks > 1                            # the maximum really occurs in several blocks
    ref = np.asarray(sim_ref.thumbnail_filter(special["dyadic"], M, band), dtype=np.float64)
    assert np.array_equal(got["dyadic"][0], ref)                 # exact window sums
    for name in ("degenerate_constant", "degenerate_max_is_min"):            # the unmasked maximum is the fill value: a masked cell is first
        filt, pos, _ = got[name]
        assert np.all(filt == filt[0, 0]) and pos == (0, 0), name
    assert np.isnan(got["nan_all"][0]).all() and got["nan_all"][1] == (0, 0)
    for name in ("nan_run_start", "nan_mid_run", "nan_run_end", "nan_row_and_column"):
        filt = got[name][0]
        assert np.isnan(filt[sim_ref.mask(filt.shape[0], band, 0, 1)]).all() and not np.isnan(filt).all()


@pytest.mark.parametrize("band_name", sim_ref.THUMB_BANDS)
def test_band_masks_at_batch_level(gpu_lib, band_name):
    ns, M = (40, 100, 287), 5
    band = sim_ref.band_value(band_name, ns[1] - M + 1)          # "R" and "R + 5" are those of the middle clip
    mats = [cases.symmetric_matrix(n, 400 + n) for n in ns]
    out = _check_against_single(gpu_lib, mats, ["band%d" % n for n in ns], M, band)
    for (filt, _, _), n in zip(out, ns):
        masked = sim_ref.mask(n - M + 1, band, 0, 1)
        assert np.all(filt[masked] == filt.min())


@pytest.mark.parametrize("R,l1,l2", sim_ref.THUMB_TRUNC)
def test_limit_truncation_at_batch_level(gpu_lib, R, l1, l2):
    """limit * R just below / at / just above an integer: the clip with that R sits between two others"""
    M = 6
    ns = (57, R + M - 1, 131)
    mats = [cases.symmetric_matrix(n, 500 + n) for n in ns]
    out = _check_against_single(gpu_lib, mats, ["trunc%d" % n for n in ns], M, 2.0, l1, l2)
    for (filt, _, _), n in zip(out, ns):
        masked = sim_ref.mask(n - M + 1, 2.0, l1, l2)             # Python's int(limit * R)
        assert np.all(filt[masked] == filt.min())
        assert (~masked).sum() < 2 or np.any(filt[~masked] != filt.min())            # what the limits leave was not overwritten


# ---- stage 5: grow ---------------------------------------------------------------------------------------------------------------------
def test_grow_on_the_device_walks_like_the_host(gpu_lib):
    """constructed matrices that end the walk by each break condition (tests/thumb_batch_cases.py, asserted there without a
    device), as clips of one batch with ordinary clips between them"""
    grow = cases.grow_cases()
    names, mats = [], []
    for k, (name, (S, _, _)) in enumerate(grow.items()):
        names += [name, "sym%d" % (61 + k)]
        mats += [S, cases.symmetric_matrix(61 + k, 600 + k)]
    out = _check_against_single(gpu_lib, mats, names, cases.GROW_M, 0.0)
    for name, (filt, pos, bounds) in zip(names, out):
        if name in grow:
            _, want_pos, (stop, back, fwd, ties) = grow[name]
            assert pos == want_pos, (name, pos)
            assert cases.walk(filt, pos[0], pos[1], cases.GROW_M) == (bounds, back, fwd, ties, stop), name


# ---- stale scratch and chunk seams -----------------------------------------------------------------------------------------------------
def test_chunk_seams_and_stale_scratch_do_not_change_a_bit(gpu_lib):
    """The same batch under the default chunk_bytes, one clip per chunk, a split between clips 2 and 3, and after a larger batch
    has left its matrices, candidates and lists in the scratch.  A 68-row clip of 100 vectors needs about 0.3 MB of scratch
    (Z 70 KB, features 54 KB, matrices 80 + 72 KB), one of 400 vectors about 3 MB: under 2 MB the clips 0 .. 2 fill a chunk
    of 0.9 MB that clip 3 does not fit into, and clip 3 is a chunk of its own."""
    Ts, M = (100, 90, 110, 400, 100), 8
    mats = [sim_ref.seeded_features(68, t, seed=7) for t in Ts]
    base = aS.thumbnail_batch(mats, M, BAND)
    for c, (f, (filt, pos, bounds)) in enumerate(zip(mats, base)):       # the batch itself: every clip equals paa_thumbnail_f64
        want = np.empty_like(filt)
        want_pos = np.zeros(2, dtype=np.int64)
        _ffi.check(gpu_lib.paa_thumbnail_f64(_ffi.as_f64p(f), 68, f.shape[1], M, BAND, 0.0, 1.0, _ffi.as_f64p(want), _ffi.as_i64p(want_pos)))
        _nan_equal_bits(filt, want, "clip %d" % c)
        assert pos == (int(want_pos[0]), int(want_pos[1])) and bounds == aS._grow_thumbnail(filt, pos[0], pos[1], M)
    sims = aS.self_similarity_batch(mats)

    def same(other, what):
        for c, (a, b) in enumerate(zip(base, other)):
            _nan_equal_bits(a[0], b[0], "%s, clip %d" % (what, c))
            assert a[1:] == b[1:], (what, c)
    same(aS.thumbnail_batch(mats, M, BAND, chunk_bytes=1), "one clip per chunk")
    same(aS.thumbnail_batch(mats, M, BAND, chunk_bytes=2 << 20), "split between clips 2 and 3")
    bigger = [sim_ref.seeded_features(68, t, seed=8) for t in (500, 300, 129, 450, 260, 200, 130)]
    aS.thumbnail_batch(bigger, 3, 1.0, 0.2, 0.7)
    same(aS.thumbnail_batch(mats, M, BAND), "after a larger batch")
    for chunk in (1, 2 << 20):
        for c, (a, b) in enumerate(zip(sims, aS.self_similarity_batch(mats, chunk_bytes=chunk))):
            _nan_equal_bits(a, b, "similarity, chunk_bytes %d, clip %d" % (chunk, c))
        same(aS.thumbnail_filter_batch(sims, M, BAND, chunk_bytes=chunk), "filter stage, chunk_bytes %d" % chunk)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN_DIR, "thumb_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_music_thumbnailing_batch_end_to_end(gpu_lib, path):
    g = load_golden(path)
    fs, seed = g["fs"], int(g["seed"])
    sw, ss, th = float(g["short_window"]), float(g["short_step"]), float(g["thumb_size"])
    l1, l2 = float(g["limit_1"]), float(g["limit_2"])
    m = int(round(th / ss))
    clips = [synth_song(seed + 1, 15.0, fs), synth_song(seed, float(g["seconds"]), fs), synth_song(seed + 2, 21.0, fs)]
    out = aS.music_thumbnailing_batch(clips, fs, sw, ss, th, l1, l2, return_filtered=True, return_details=True)
    # the golden's clip, in the middle of the batch, against the unmodified reference
    a1, a2, b1, b2, filt, pos = out[1]
    assert filt.shape == g["filtered"].shape and np.array_equal(np.isnan(filt), np.isnan(g["filtered"]))
    d = float(np.abs(np.nan_to_num(filt) - np.nan_to_num(g["filtered"])).max())
    print("%s: max abs diff to the golden %g (gate %g)" % (os.path.basename(path), d, 2e-5 * m))
    assert d <= 2e-5 * m
    assert [a1, a2, b1, b2] == list(g["pos"])
    # every clip against its own single call
    for c, x in enumerate(clips):
        s1, s2, t1, t2, want = aS.music_thumbnailing(x, fs, sw, ss, th, l1, l2)
        a1, a2, b1, b2, filt, pos = out[c]
        print("clip %d: max abs diff to its single call %g" % (c, float(np.abs(np.nan_to_num(filt) - np.nan_to_num(want)).max())))
        _nan_equal_bits(filt, want, "clip %d" % c)
        assert (a1, a2, b1, b2) == (s1, s2, t1, t2), c
        assert pos == sim_ref.argmax_margin(want)[0], c
    # one clip per chunk (one plan each), and the times alone: nothing but 48 bytes per clip comes back
    alone = aS.music_thumbnailing_batch(clips, fs, sw, ss, th, l1, l2, chunk_bytes=1)
    assert alone == [o[:4] for o in out]
    # the packed form of the entry point (Python passes one pointer per clip): the same arg-max cells and bounds
    packed = np.concatenate(clips)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in clips])]).astype(np.int64)
    p, b = np.zeros((3, 2), dtype=np.int64), np.zeros((3, 4), dtype=np.int64)
    _ffi.check(gpu_lib.paa_music_thumbnail_batch_i16(_ffi.as_i16p(packed), _ffi.as_i64p(offsets), 3, float(fs), int(fs * sw), int(fs * ss), m,
                                                     5.0 / ss, l1, l2, 0, _ffi.as_i64p(p), _ffi.as_i64p(b), None))
    assert [tuple(r) for r in p.tolist()] == [o[5] for o in out]
    assert [(ss * r[0], ss * r[1], ss * r[2], ss * r[3]) for r in b.tolist()] == [o[:4] for o in out]


# ---- sample types ------------------------------------------------------------------------------------------------------------------------
def test_each_sample_type_takes_the_path_of_its_single_call(gpu_lib):
    x = synth_song(35, 12.0, 8000)
    assert x.dtype == np.int16
    clips = [x, np.double(x), np.stack([x, x], axis=1), np.float32(x[:72000])]
    out = aS.music_thumbnailing_batch(clips, 8000, 0.5, 0.25, 2.0, return_filtered=True)
    for c, sig in enumerate(clips):
        want = aS.music_thumbnailing(sig, 8000, 0.5, 0.25, 2.0)
        assert out[c][:4] == want[:4], c
        _nan_equal_bits(out[c][4], want[4], "clip %d" % c)


def test_files_come_back_in_path_order(gpu_lib, tmp_path):
    import scipy.io.wavfile as wavfile
    songs = [(8000, synth_song(41, 12.0, 8000)), (16000, synth_song(42, 9.0, 16000)), (8000, synth_song(43, 10.0, 8000))]
    paths = []
    for k, (fs, x) in enumerate(songs):
        paths.append(str(tmp_path / ("song%d.wav" % k)))
        wavfile.write(paths[-1], fs, x)
    out = aS.music_thumbnailing_files(paths, 0.5, 0.25, 2.0, return_filtered=True)
    assert len(out) == 3
    for k, (fs, x) in enumerate(songs):
        want = aS.music_thumbnailing(x, fs, 0.5, 0.25, 2.0)
        assert out[k][:4] == want[:4], k
        _nan_equal_bits(out[k][4], want[4], "file %d" % k)
    assert out[0][4].shape != out[2][4].shape                    # the two 8 kHz files are told apart by their lengths


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_clip_and_nothing_has_run(gpu_lib, monkeypatch):
    """the refusals come from the argument half: the library entry points of the batch are never called"""
    def reached(*a, **k):
        raise AssertionError("the batch reached the library")
    monkeypatch.setattr(aS, "_thumb_group", reached)
    ok = synth_song(36, 12.0, 8000)
    with pytest.raises(ValueError, match=r"clip 2: need at least one array to concatenate"):
        aS.music_thumbnailing_batch([ok, ok, ok[:3999]], 8000, 0.5, 0.25, 2.0)
    with pytest.raises(ValueError, match=r"clip 1: 5 feature vectors are fewer than the thumbnail filter length 8"):
        aS.music_thumbnailing_batch([ok, ok[:12000], ok], 8000, 0.5, 0.25, 2.0)
    monkeypatch.undo()
    # and the library itself refuses the same batches before any device work: its outputs stay as they were
    packed = np.concatenate([ok, ok[:12000]])
    offsets = np.array([0, len(ok), len(packed)], dtype=np.int64)
    pos, bounds = np.full((2, 2), -5, dtype=np.int64), np.full((2, 4), -5, dtype=np.int64)
    rc = gpu_lib.paa_music_thumbnail_batch_i16(_ffi.as_i16p(packed), _ffi.as_i64p(offsets), 2, 8000.0, 4000, 2000, 8, 20.0, 0.0, 1.0, 0,
                                               _ffi.as_i64p(pos), _ffi.as_i64p(bounds), None)
    assert rc == _ffi.ERR_ARG and "clip 1" in _ffi.last_error()
    assert np.all(pos == -5) and np.all(bounds == -5)
