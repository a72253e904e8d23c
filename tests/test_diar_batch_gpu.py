"""diarize_features_batch / speaker_diarization_batch on the GPU: clip i of any batch must EQUAL its own single call
(diarize_features / speaker_diarization_signal) bit for bit -- kept_dims; per k labels, centers, n_iter, inertia, sil_a, sil_b,
sil and pair_sums; scores; imax; hmm_states; the filtered labels -- at any position, beside any other clips, under any
chunk_bytes and for every way of seeding.  One single call per distinct (clip, n_speakers, seed) is cached for the module.  The
golden clips still pass the reference gates of tests/test_diar_gpu.py from inside a batch.  -m gpu."""
import os

import numpy as np
import pytest

import diar_batch_cases as cases
import test_diar_gpu as single_tests
from conftest import golden_id, load_golden
from pyaudioanalysis_amd import audioSegmentation as aS

pytestmark = pytest.mark.gpu

SEED = 7
_single_cache = {}


def single(key, M, n_speakers, seed=SEED, init=None):
    """diarize_features of one clip with an int seed (or given centres): (cls, details), or the exception it raises"""
    k = (key, int(n_speakers), seed, None if init is None else tuple(sorted(init)))
    if k not in _single_cache:
        try:
            _single_cache[k] = aS.diarize_features(M, n_speakers, random_state=seed, init_centers=init, return_details=True)
        except (ValueError, IndexError) as exc:
            _single_cache[k] = exc
    return _single_cache[k]


def single_clusters(key, M, n_speakers, seed=SEED, init=None):
    """diarize_clusters_device of one clip: the clustering half of the details, for a clip whose HMM refuses its labels"""
    from pyaudioanalysis_amd import _ffi
    k = ("clusters", key, int(n_speakers), seed, None if init is None else tuple(sorted(init)))
    if k not in _single_cache:
        d_m = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(M, dtype=np.float64))
        try:
            _single_cache[k], d_z = aS.diarize_clusters_device(d_m, M.shape[0], M.shape[1], n_speakers, random_state=seed, init_centers=init)
            d_z.free()
        finally:
            d_m.free()
    return _single_cache[k]


def assert_same_outcome(got, entry, seed, what):
    """one slot of a batch run with on_error="record" against the single call of its clip: the same result bit for bit, or the
    same exception -- and when it was the HMM that refused, the same clustering details on the exception"""
    key, M, n_speakers, init = entry
    want = single(key, M, n_speakers, seed, init)
    if not isinstance(want, BaseException):
        assert not isinstance(got, BaseException), (what, got)
        cases.assert_same_result(got, want, what)
        return True
    assert type(got) is type(want) and str(got) == str(want), (what, got, want)
    if getattr(got, "details", None) is not None:
        cases.assert_same_clusters(got.details, single_clusters(key, M, n_speakers, seed, init), what)
    return False


def check_batch(entries, seed=SEED, **kw):
    """entries: (key, M, n_speakers, init or None) per clip.  One batch with an int seed against the single call of every clip
    (a tiny clip's last k leaves one-window clusters, which the HMM refuses: then the exceptions and the clustering must agree)."""
    inits = [e[3] for e in entries]
    out = aS.diarize_features_batch([e[1] for e in entries], [e[2] for e in entries], random_state=seed,
                                    init_centers=inits if any(i is not None for i in inits) else None, return_details=True,
                                    on_error="record", **kw)
    assert len(out) == len(entries)
    good = [assert_same_outcome(out[c], e, seed, "clip %d (%s)" % (c, e[0])) for c, e in enumerate(entries)]
    return out, good


@pytest.fixture(scope="module")
def ragged(gpu_lib):
    """per n_dims the ragged clips, every one with the sweep; at 9 dims also the two clips past NumPy's summation chunks, k = 3"""
    out = {}
    for d in cases.DIMS:
        entries = [("ragged%d_%d" % (d, M.shape[1]), M, 0, None) for M in cases.ragged_clips(d)]
        if d == 9:
            entries += [("big%d" % n, cases.planted(n, n, d, 3), 3, None) for n in cases.BIG_N]
        out[d] = entries
    return out


# ---- ragged batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", cases.DIMS)
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_ragged_batch_equals_the_single_calls(ragged, d, order):
    entries = ragged[d][::-1] if order == "reversed" else ragged[d]
    out, good = check_batch(entries)
    assert sum(good) >= len(entries) - 3                              # all but the tiniest clips go through the HMM
    kept = {len(o[1]["kept_dims"]) for o, ok in zip(out, good) if ok}
    assert len(kept) > 1                                              # the kept-dimension counts differ inside the batch


@pytest.mark.parametrize("d", cases.DIMS)
def test_every_clip_alone_as_a_batch_of_one(ragged, d):
    for e in ragged[d]:
        check_batch([e])


@pytest.mark.parametrize("d", [9, 148])
def test_chunk_bytes_do_not_show(ragged, d):
    entries = ragged[d]
    need = [aS._diar_clip_bytes(d, e[1].shape[1], aS._diar_batch_ks(e[2])) for e in entries]
    ns = [e[1].shape[1] for e in entries]
    ks_list = [aS._diar_batch_ks(e[2]) for e in entries]
    assert len(aS._diar_batch_chunks(d, ns, ks_list, 1)) == len(entries)
    check_batch(entries, chunk_bytes=1)                               # one clip per chunk
    half = sum(need[:len(need) // 2])
    chunks = aS._diar_batch_chunks(d, ns, ks_list, half)
    assert 1 < len(chunks) < len(entries) and chunks[0] == (0, len(need) // 2)
    check_batch(entries, chunk_bytes=half)                            # split in the middle


# ---- per-clip n_speakers --------------------------------------------------------------------------------------------------------------
def test_fixed_k_beside_the_sweep(gpu_lib):
    """k = 2, 8, 9, 16, 17, 32 -- both sides of the assign kernel's 8 / 16 / 32 instances -- on one clip of 257 windows, mixed with
    sweeps of other clips: the instance a job runs in is chosen by the LARGEST k of its chunk, and must not show"""
    M = cases.planted(77, 257, 33, 6)
    other = cases.planted(78, 130, 33, 3)
    entries = []
    for k in cases.FIXED_KS:
        entries += [("fixed", M, k, None), ("other", other, 0, None)]
    check_batch(entries)                                              # the largest k is 32: every job in the 32-wide instance
    check_batch([("fixed", M, 2, None), ("other", other, 3, None), ("fixed", M, 8, None)])      # k <= 8 only: the 8-wide instance
    check_batch([("fixed", M, 9, None), ("other", other, 0, None), ("fixed", M, 16, None)])     # 9 .. 16: the 16-wide instance
    check_batch(entries[:8], chunk_bytes=1)                           # every job in the instance of its own k


# ---- seeds ----------------------------------------------------------------------------------------------------------------------------
def _loop(mats, speakers, rs, inits=None):
    """the loop of single calls under one random_state object: per clip the result or the exception"""
    out = []
    for c, (M, s) in enumerate(zip(mats, speakers)):
        try:
            out.append(aS.diarize_features(M, s, random_state=rs, init_centers=None if inits is None else inits[c], return_details=True))
        except (ValueError, IndexError) as exc:
            out.append(exc)
    return out


def _same_outcomes(got, want):
    """slot by slot: the same result bit for bit, or the same exception; returns how many clips went through"""
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, BaseException):
            assert type(g) is type(w) and str(g) == str(w), (c, g, w)
        else:
            assert not isinstance(g, BaseException), (c, g)
            cases.assert_same_result(g, w, "clip %d" % c)
    return sum(not isinstance(w, BaseException) for w in want)


def test_shared_random_state_is_consumed_as_the_loop_consumes_it(gpu_lib):
    mats = [cases.planted(200 + i, n, 9, 3) for i, n in enumerate((140, 129, 9, 300))]
    speakers = [0, 4, 0, 2]
    want = _loop(mats, speakers, np.random.RandomState(5))
    rs = np.random.RandomState(5)
    got = aS.diarize_features_batch(mats, speakers, random_state=rs, return_details=True, on_error="record")
    assert _same_outcomes(got, want) >= 2
    ref = np.random.RandomState(5)
    _loop(mats, speakers, ref)
    assert rs.randint(1 << 30) == ref.randint(1 << 30)               # and the state stands where the loop leaves it
    split = aS.diarize_features_batch(mats, speakers, random_state=np.random.RandomState(5), return_details=True, chunk_bytes=1,
                                      on_error="record")
    _same_outcomes(split, want)


def _goldens(n_dims=None):
    out = []
    for p in single_tests.GOLDENS:
        g = load_golden(p)
        if n_dims is None or g["M"].shape[0] == n_dims:
            out.append((golden_id(p), g))
    return out


def test_given_centres_do_not_shift_the_other_clips_draws(gpu_lib):
    """golden clips with their stored initial centres (no draw at all) between seeded clips, under one shared RandomState"""
    real = _goldens(148)
    mats, speakers, inits = [], [], []
    for i, (name, g) in enumerate(real):
        mats += [cases.planted(300 + i, 160 + 7 * i, 148, 3), g["M"]]
        speakers += [0, 0]
        inits += [None, single_tests.init_of(g)]
    partial = single_tests.init_of(real[0][1])
    mats.append(real[0][1]["M"])                                       # and one whose k = 4 alone is given: seven k are drawn
    speakers.append(0)
    inits.append({4: partial[4]})
    want = _loop(mats, speakers, np.random.RandomState(9), inits)
    got = aS.diarize_features_batch(mats, speakers, random_state=np.random.RandomState(9), init_centers=inits, return_details=True,
                                    on_error="record")
    assert _same_outcomes(got, want) >= len(real)


# ---- goldens inside a batch -----------------------------------------------------------------------------------------------------------
def _golden_gates(name, g, cls, det):
    """the gates of test_cluster_stages_match_golden and test_diarize_features_matches_golden (k = 9: the sweep)"""
    close, FLOOR = single_tests.assert_close, single_tests.DIST_FLOOR
    close(det["mean"], g["mean"], "mean")
    close(det["scale"], g["scale"], "scale")
    close(det["dim_colsum"], g["colsum"], "dimension distance sums")
    assert float(g["kept_margin"]) >= FLOOR and np.array_equal(det["kept_dims"], g["kept_dims"])
    excluded = 0
    for k in (int(k) for k in g["ks"]):
        pre = "k%d_" % k
        if float(g[pre + "km_margin"]) < FLOOR or float(g[pre + "b_margin"]) < FLOOR:
            excluded += 1
            continue
        assert np.array_equal(det["labels"][k], g[pre + "labels"]) and det["n_iter"][k] == int(g[pre + "n_iter"]), k
        for key, stored in (("centers", "centers"), ("inertia", "inertia"), ("pair_sums", "pair_sums"), ("sil_a", "a"), ("sil_b", "b"),
                            ("sil", "sil")):
            close(det[key][k], g[pre + stored], "%s k=%d" % (key, k))
    assert excluded == 0 if name in single_tests.REAL else excluded < len(g["ks"])
    if excluded == 0:
        close(det["scores"], g["scores"], "scores")
        assert float(g["imax_margin"]) >= FLOOR and det["imax"] == int(g["imax"])
    if 9 in [int(k) for k in g["hmm_ks"]]:
        assert float(g["k9_hmm_margin"]) >= single_tests.HMM_FLOOR and float(g["k9_km_margin"]) >= FLOOR
        assert np.array_equal(det["hmm_states"], g["k9_hmm_states"])
        assert cls.dtype == np.float64 and np.array_equal(cls, g["k9_cls"])
        if "flags_gt" in g:
            got = aS.evaluate_speaker_diarization(cls, g["flags_gt"])
            assert got[0] == g["k9_purity"][0] and got[1] == g["k9_purity"][1]


@pytest.mark.parametrize("n_dims", [148, 40])
def test_golden_clips_pass_the_reference_gates_inside_a_batch(gpu_lib, n_dims):
    goldens = _goldens(n_dims)
    assert len(goldens) == (3 if n_dims == 148 else 1)
    entries = [("filler%d" % n_dims, cases.planted(400 + n_dims, 231, n_dims, 4), 4, None)]
    for name, g in goldens:
        entries += [(name, g["M"], 0, single_tests.init_of(g)), ("filler%d_%s" % (n_dims, name), cases.planted(len(name), 77, n_dims, 2), 3, None)]
    out, good = check_batch(entries)
    assert all(good[1::2])                                            # every golden clip went through the HMM
    for (name, g), (cls, det) in zip(goldens, out[1::2]):
        _golden_gates(name, g, cls, det)


# ---- failures -------------------------------------------------------------------------------------------------------------------------
def _failing_batches():
    const = [g for name, g in _goldens(12) if name == "diar_const"][0]
    empty_M, empty_init = cases.empty_cluster_clip(9)
    a = [("good12a", cases.planted(501, 160, 12, 3), 3, None), ("diar_const", const["M"], 0, single_tests.init_of(const)),
         ("good12b", cases.planted(502, 140, 12, 2), 3, None)]
    b = [("good9a", cases.planted(503, 150, 9, 3), 3, None), ("no_kept", cases.no_kept_dimension_clip(9), 3, None),
         ("good9b", cases.planted(504, 129, 9, 2), 2, None), ("empty_cluster", empty_M, 3, empty_init),
         ("good9c", cases.planted(505, 133, 9, 2), 2, None)]
    return (a, {1: ValueError}), (b, {1: ValueError, 3: IndexError})


@pytest.mark.parametrize("which", [0, 1])
def test_failing_clips_are_recorded_and_leave_their_neighbours_intact(gpu_lib, which):
    entries, failing = _failing_batches()[which]
    for c, kind in failing.items():
        want = single(*entries[c][:3], SEED, entries[c][3])
        assert type(want) is kind, (entries[c][0], want)               # the loop raises exactly this
    inits = [e[3] for e in entries]
    args = ([e[1] for e in entries], [e[2] for e in entries])
    out = aS.diarize_features_batch(*args, random_state=SEED, init_centers=inits, return_details=True, on_error="record")
    for c, e in enumerate(entries):
        assert assert_same_outcome(out[c], e, SEED, "clip %d (%s)" % (c, e[0])) == (c not in failing)
    first = min(failing)
    with pytest.raises(failing[first], match="clip %d: " % first):
        aS.diarize_features_batch(*args, random_state=SEED, init_centers=inits)
    with pytest.raises(failing[first], match="clip %d: " % first):
        aS.diarize_features_batch(*args, random_state=SEED, init_centers=inits, chunk_bytes=1)


def test_wrong_width_of_given_centres_is_the_loops_error(gpu_lib):
    """[k][kept dims] is known only after the filter: a width that is not the kept dims raises where the loop raises, after the
    draws of the k before it, and the clips behind it draw what they would have drawn"""
    mats = [cases.planted(600 + i, 150 + i, 9, 3) for i in range(3)]
    inits = [None, {4: np.zeros((4, 1))}, None]
    rs_loop, want = np.random.RandomState(2), []
    for M, init in zip(mats, inits):
        try:
            want.append(aS.diarize_features(M, 0, random_state=rs_loop, init_centers=init, return_details=True))
        except ValueError as exc:
            want.append(exc)
        except IndexError as exc:
            want.append(exc)
    assert isinstance(want[1], ValueError) and "init_centers[4]" in str(want[1])
    got = aS.diarize_features_batch(mats, 0, random_state=np.random.RandomState(2), init_centers=inits, return_details=True,
                                    on_error="record")
    assert _same_outcomes(got, want) >= 1


# ---- stage functions ------------------------------------------------------------------------------------------------------------------
def test_stage_functions_alone(gpu_lib):
    from pyaudioanalysis_amd import _ffi
    mats = [cases.planted(700 + i, n, 9, 3) for i, n in enumerate((140, 257, 130))]
    ns = np.array([m.shape[1] for m in mats])
    cols = np.concatenate(([0], np.cumsum(ns)[:-1]))
    d_m = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(np.concatenate(mats, axis=1)))
    try:
        results, d_z = aS.diarize_clusters_batch_device(d_m, 9, int(ns.sum()), cols, ns, [0, 3, 0], random_state=SEED)
        try:
            states = aS.diarize_hmm_batch_device(d_z, 9, int(ns.sum()), cols, ns, [r["labels"][r["ks"][-1]] for r in results])
            Z = d_z.to_host(np.float64, 9 * int(ns.sum())).reshape(9, -1)
        finally:
            d_z.free()
    finally:
        d_m.free()
    for c, M in enumerate(mats):
        d_one = _ffi.DeviceBuffer.from_host(M)
        try:
            want, d_zone = aS.diarize_clusters_device(d_one, 9, M.shape[1], [0, 3, 0][c], random_state=SEED)
            z_one = d_zone.to_host(np.float64, M.size).reshape(M.shape)
            d_zone.free()
        finally:
            d_one.free()
        assert cases.same_bits(Z[:, cols[c]:cols[c] + ns[c]], z_one)
        for k in want["ks"]:
            for key in ("labels", "centers", "sil", "pair_sums"):
                assert cases.same_bits(results[c][key][k], want[key][k]), (c, key, k)
        whole = single("stage%d" % c, M, [0, 3, 0][c])
        if isinstance(whole, BaseException):
            assert type(states[c]) is type(whole) and str(states[c]) == str(whole)
        else:
            assert cases.same_bits(states[c], whole[1]["hmm_states"])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _signals():
    from synth import synth_clip
    fs = 16000
    a = np.concatenate([synth_clip(s, 2 * fs) for s in (1, 2, 3, 1, 2, 3, 1)])
    b = np.concatenate([synth_clip(s, 2 * fs) for s in (4, 5, 9, 4, 5, 9)])
    c = np.concatenate([synth_clip(s, 2 * fs, stereo=True) for s in (6, 7, 8, 6, 7, 8, 6, 7)])
    return fs, [a, c, b.astype(np.float64)]


def _signal_clusters(x, fs, n_speakers, models, seed):
    """the clustering half of speaker_diarization_signal, by its own steps in its own order (the mid-term matrix on the device,
    the two SVMs' probabilities + 1e-4 below it, diarize_clusters_device): what the loop computed before its HMM refused"""
    import ctypes as C
    from pyaudioanalysis_amd import _ffi, audioBasicIO, audioTrainTest
    svcs = [(audioTrainTest.svc_model(m[0]), np.asarray(m[1], dtype=np.float64), np.asarray(m[2], dtype=np.float64)) for m in models]
    st = round(fs * 0.05)
    extra = sum(len(s[0].classes) for s in svcs)
    with aS._mid_term_on_device(audioBasicIO.stereo_to_mono(x), fs, 1.0, 0.1, st, st, extra) as (d_all, M):
        at = 136
        for model, mean, std in svcs:
            _, proba = model.predict_device(d_all, M, M, mean, std)
            block = np.ascontiguousarray(proba.T + 1e-4)
            _ffi.check(_ffi.lib().paa_memcpy_h2d(C.c_void_p(d_all.ptr.value + at * M * 8), block.ctypes.data_as(C.c_void_p), block.nbytes))
            at += block.shape[0]
        details, d_z = aS.diarize_clusters_device(d_all, 136 + extra, M, n_speakers, random_state=seed)
        d_z.free()
    return details


def test_speaker_diarization_batch_equals_the_loop(gpu_lib):
    """three signals of different lengths -- int16, stereo int16 and float64 -- against the loop of speaker_diarization_signal.  A
    signal whose SVM probability row is constant over a cluster is refused by the HMM in the loop and in the batch alike: then
    the exceptions agree and the clustering on the batch's exception equals the loop's clustering steps bit for bit."""
    fs, signals = _signals()
    models = single_tests.synthetic_models()
    speakers = [3, 2, 2]
    want = []
    for x, s in zip(signals, speakers):
        try:
            want.append(aS.speaker_diarization_signal(x, fs, s, models=models, random_state=4, return_details=True))
        except ValueError as exc:
            want.append(exc)
    got = aS.speaker_diarization_batch(signals, fs, speakers, models=models, random_state=4, return_details=True, on_error="record")
    assert _same_outcomes(got, want) >= 2
    for c in range(3):
        if isinstance(want[c], BaseException):
            assert got[c].details is not None
            cases.assert_same_clusters(got[c].details, _signal_clusters(signals[c], fs, speakers[c], models, 4), "signal %d" % c)
    plain = aS.speaker_diarization_batch(signals[::-1], fs, speakers[::-1], models=models, random_state=4, chunk_bytes=1,
                                         on_error="record")
    for c in range(3):
        if not isinstance(want[c], BaseException):
            assert cases.same_bits(plain[2 - c], want[c][0])
        else:
            assert type(plain[2 - c]) is type(want[c]) and str(plain[2 - c]) == str(want[c])


def _folder(tmp_path, all_segments=False):
    from scipy.io import wavfile
    from synth import synth_clip
    paths = []
    for name, fs, seeds in (("a", 16000, (1, 2, 1, 2, 1, 2)), ("b", 8000, (3, 4, 3, 4, 3, 4, 3)), ("c", 16000, (5, 6, 5, 6, 5))):
        x = np.concatenate([synth_clip(s, 2 * fs, fs=fs) for s in seeds])
        paths.append(str(tmp_path / ("%s.wav" % name)))
        wavfile.write(paths[-1], fs, x)
    for name in ("a", "b", "c") if all_segments else ("a",):
        with open(str(tmp_path / ("%s.segments" % name)), "w") as f:
            for i in range(5):
                f.write("%d\t%d\tspeaker%d\n" % (2 * i, 2 * i + 2, i % 2))
    return paths


def test_files_and_evaluation_equal_the_loop(gpu_lib, tmp_path, capsys):
    paths = _folder(tmp_path)
    models = single_tests.synthetic_models()
    want = [aS.speaker_diarization(p, 2, models=models, random_state=3) for p in paths]
    loop_out = capsys.readouterr().out
    got = aS.speaker_diarization_files(paths, 2, models=models, random_state=3)
    assert capsys.readouterr().out == loop_out and loop_out.count("\t") == 1
    for (w_cls, w_pc, w_ps), (g_cls, g_pc, g_ps) in zip(want, got):
        assert cases.same_bits(w_cls, g_cls) and w_pc == g_pc and w_ps == g_ps
    assert want[0][1] >= 0 and want[1][1] == -1
    shared = [aS.speaker_diarization(p, 2, models=models, random_state=rs) for rs in [np.random.RandomState(8)] for p in paths]
    capsys.readouterr()
    by_files = aS.speaker_diarization_files(paths, 2, models=models, random_state=np.random.RandomState(8))
    capsys.readouterr()
    for w, g in zip(shared, by_files):                                # two rates: the draws still follow the PATH order
        assert cases.same_bits(w[0], g[0])
    folder = tmp_path / "evaluation"                                  # every file with its ground truth: two speakers, no sweep
    folder.mkdir()
    _folder(folder, all_segments=True)
    aS.speaker_diarization_evaluation(str(folder), [0], models=models, random_state=3, batch=False)
    loop_lines = capsys.readouterr().out
    aS.speaker_diarization_evaluation(str(folder), [0], models=models, random_state=3, batch=True)
    assert capsys.readouterr().out == loop_lines and "LDA = 0" in loop_lines and loop_lines.count("\t") == 3


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_a_batch_are_bit_identical(ragged):
    entries = ragged[33]
    runs = [aS.diarize_features_batch([e[1] for e in entries], 0, random_state=11, return_details=True, on_error="record")
            for _ in range(2)]
    assert _same_outcomes(runs[0], runs[1]) >= len(entries) - 3
