"""silence_removal_batch on the GPU (pyaudioanalysis_amd/csrc/kernels_onset.hpp, lib_onset.hpp): the stages against NumPy and the
restatement tests/onset_ref.py, the whole call against the reference's goldens and against a loop of the existing host
functions, and its invariance under batch position and chunking.  -m gpu.  The margins these comparisons rely on are asserted on
the CPU in tests/test_onset_batch_cpu.py for every input used here."""
import os
import sys

import numpy as np
import pytest

import onset_ref
from conftest import GOLDEN_DIR
from pyaudioanalysis_amd import ShortTermFeatures as stf, audioSegmentation as aS, audioTrainTest as aT

pytestmark = pytest.mark.gpu

TIGHT = 1e-9          # the project's tight gate for probabilities


def load(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def same_record(a, b, keys):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


STAGE12_KEYS = ("quiet_limit", "loud_limit", "quiet_idx", "loud_idx", "features", "mean", "scale")
DETAIL_KEYS = ("quiet_idx", "loud_idx", "quiet_limit", "loud_limit", "mean", "scale", "seed", "alpha_y", "rho", "prob_a", "prob_b",
               "n_sv", "status", "iterations", "raw_prob", "prob", "threshold", "active")


# ---- stages 1 and 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", onset_ref.STAGE1_KINDS)
def test_selection_and_training_sets_against_numpy(gpu_lib, kind):
    mats = [onset_ref.stage1_case(kind, T) for T in onset_ref.STAGE1_FRAMES]
    got = aS.onset_training_sets(mats)
    for st, g in zip(mats, got):
        T = st.shape[1]
        ref = onset_ref.training_sets(st)
        ranked, tenth = np.sort(st[1]), T // 10
        for mine, theirs in ((g["quiet_limit"], ranked[:tenth].mean() + 1e-15), (g["loud_limit"], ranked[-tenth:-1].mean() + 1e-15)):
            print(kind, T, mine, theirs, abs(mine - theirs) / theirs)
            if kind in onset_ref.EXACT_KINDS:
                assert mine == theirs, (kind, T)
            else:
                assert abs(mine - theirs) <= onset_ref.limit_bound(tenth) * theirs, (kind, T)
        assert np.array_equal(g["quiet_idx"], ref["quiet_idx"]) and np.array_equal(g["loud_idx"], ref["loud_idx"]), (kind, T)
        assert np.array_equal(g["quiet_flags"], st[1] <= ref["quiet_limit"]) and np.array_equal(g["loud_flags"], st[1] >= ref["loud_limit"])
        quiet, loud = aS._energy_extremes(st)
        feats = np.vstack([quiet.T, loud.T])
        assert np.array_equal(g["features"], feats), (kind, T)
        assert np.array_equal(g["mean"], ref["mean"]) and np.array_equal(g["scale"], ref["scale"]), (kind, T)
        if len(feats) >= 3:             # NumPy's own reductions, bit for bit
            scale = np.sqrt(feats.var(axis=0))
            scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
            assert np.array_equal(g["mean"], feats.mean(axis=0)) and np.array_equal(g["scale"], scale), (kind, T)
        if kind == "all_equal":         # counts are reported; the whole call refuses such a clip (test_an_empty_set_names_the_clip)
            assert len(g["quiet_idx"]) == T and len(g["loud_idx"]) == 0
        if kind == "overlap":
            assert len(g["quiet_idx"]) == T and len(g["loud_idx"]) == 1 and g["loud_idx"][0] in g["quiet_idx"]


def test_a_constant_column_gets_scale_one(gpu_lib):
    st = np.ascontiguousarray(onset_ref.stage1_case("random", 117))
    st[5] = 3.25
    g = aS.onset_training_sets([st])[0]
    assert g["scale"][5] == 1.0 and g["mean"][5] == 3.25 and np.all(g["scale"][[0, 2, 3]] != 1.0)


def test_training_sets_are_the_same_bits_anywhere_in_a_batch_and_under_any_chunking(gpu_lib):
    rng = np.random.default_rng(300)
    clip = onset_ref.stage1_case("random", 400)
    fillers = [onset_ref.stage1_case("random", int(T), base_seed=1000) for T in rng.integers(20, 61, 298)]
    batch = [clip] + fillers + [clip]
    alone = aS.onset_training_sets([clip])[0]
    whole = aS.onset_training_sets(batch)
    assert len(whole) == 300
    assert same_record(whole[0], alone, STAGE12_KEYS) and same_record(whole[299], alone, STAGE12_KEYS)
    for chunk_bytes in (1 << 20, 300000):       # about eight clips, about two clips per chunk (the clip of 400 frames alone)
        cut = aS.onset_training_sets(batch, chunk_bytes=chunk_bytes)
        assert all(same_record(a, b, STAGE12_KEYS) for a, b in zip(whole, cut)), chunk_bytes


# ---- stages 4 and 5 ---------------------------------------------------------------------------------------------------------------
def test_activity_against_the_restatement(gpu_lib):
    cases = [onset_ref.stage45_case(*c) for c in onset_ref.STAGE45_CASES]
    mats, models = [c[0] for c in cases], [c[1] for c in cases]
    widths, weights = [c[1] for c in onset_ref.STAGE45_CASES], [c[2] for c in onset_ref.STAGE45_CASES]
    got = aS.onset_activity(mats, models, widths, weights)          # per-clip widths and weights within one batch
    for (T, width, weight), g, (_, _, ref) in zip(onset_ref.STAGE45_CASES, got, cases):
        d_raw, d_prob = np.max(np.abs(g["raw_prob"] - ref["raw_prob"])), np.max(np.abs(g["prob"] - ref["prob"]))
        print(T, width, weight, d_raw, d_prob, abs(g["threshold"] - ref["threshold"]))
        assert d_raw <= TIGHT and d_prob <= TIGHT, (T, width, weight)
        assert abs(g["threshold"] - ref["threshold"]) <= 1e-12, (T, width, weight)
        assert np.array_equal(g["active"], ref["active"]), (T, width, weight)
        if width < 3:
            assert np.array_equal(g["prob"], g["raw_prob"])          # untouched
    for k, (T, width, weight) in enumerate(onset_ref.STAGE45_CASES):
        one = aS.onset_activity([mats[k]], [models[k]], width, weight)[0]
        assert same_record(one, got[k], ("raw_prob", "prob", "threshold", "active"))
    cut = aS.onset_activity(mats, models, widths, weights, chunk_bytes=60000)
    assert all(same_record(a, b, ("raw_prob", "prob", "threshold", "active")) for a, b in zip(got, cut))
    with pytest.raises(ValueError, match="clip 1: Input vector needs to be bigger than window size"):
        aS.onset_activity(mats[:2], models[:2], [3, 41], 0.5)


# ---- the whole call -----------------------------------------------------------------------------------------------------------------
def segments_array(segs):
    return np.array(segs, dtype=np.float64).reshape(-1, 2)


def test_the_two_goldens_of_one_step_in_one_batch(gpu_lib):
    a, b = load("silence_count_050_050"), load("silence_recording1_20s")
    np.random.seed(int(a["seed"]))
    segs = aS.silence_removal_batch([a["signal"], b["signal"]], 16000, 0.05, 0.05, 0.5, 0.5)
    for got, g in zip(segs, (a, b)):
        got = segments_array(got)
        assert got.shape == g["segments"].shape and np.allclose(got, g["segments"], rtol=0, atol=1e-9), (got, g["segments"])


@pytest.mark.parametrize("name", ["silence_count_020_020", "silence_synth_gaps"])
def test_the_other_goldens_as_single_clip_batches(gpu_lib, name):
    g = load(name)
    np.random.seed(int(g["seed"]))
    segs = aS.silence_removal_batch([g["signal"]], int(g["fs"]), float(g["st_win"]), float(g["st_step"]), float(g["smooth_window"]),
                                    float(g["weight"]))
    got = segments_array(segs[0])
    assert got.shape == g["segments"].shape and np.allclose(got, g["segments"], rtol=0, atol=1e-9), (got, g["segments"])


def host_loop(clips, fs, st_win, st_step, smooth_window, weight):
    """the existing host functions over feature_extraction_batch's matrices, one clip after the other"""
    mats, _ = stf.feature_extraction_batch(clips, fs, st_win * fs, st_step * fs)
    out = []
    for st in mats:
        quiet, loud = aS._energy_extremes(st)
        svm, mean, scale = aS._train_onset_svm_device(quiet.T, loud.T, None)
        raw = aS.svm_onset_probability(st, mean, scale, svm)
        prob = aS.smooth_moving_avg(raw, smooth_window / st_step)
        active = np.flatnonzero(prob > aS._onset_threshold(prob, weight))
        out.append(dict(st=st, quiet=quiet, loud=loud, mean=mean, scale=scale, seed=svm.random_seed, alpha_y=svm.fit_result.alpha_y[0],
                        rho=float(svm.fit_result.rho[0]), prob_a=float(svm.probA_[0]), prob_b=float(svm.probB_[0]), raw=raw, prob=prob,
                        segments=aS._onset_segments(active, st_step)))
    return out


@pytest.mark.parametrize("case", ["goldens", "bursts"])
def test_the_batch_equals_a_loop_of_the_host_functions(gpu_lib, case):
    if case == "goldens":
        clips = [load("silence_count_050_050")["signal"], load("silence_recording1_20s")["signal"]]
        args = (16000, 0.05, 0.05, 0.5, 0.5)
    else:
        clips = [onset_ref.burst_clip(k) for k in range(3)]
        args = (onset_ref.FS, 0.02, 0.02, 0.2, 0.4)
    np.random.seed(1234)
    want = host_loop(clips, *args)
    np.random.seed(1234)
    segs, details = aS.silence_removal_batch(clips, *args, return_details=True)
    for w, s, d in zip(want, segs, details):
        assert d["seed"] == w["seed"]
        assert np.array_equal(w["st"][:, d["quiet_idx"]], w["quiet"]) and np.array_equal(w["st"][:, d["loud_idx"]], w["loud"])
        assert np.array_equal(d["mean"], w["mean"]) and np.array_equal(d["scale"], w["scale"])
        assert np.array_equal(d["alpha_y"], w["alpha_y"]) and d["rho"] == w["rho"]
        assert d["prob_a"] == w["prob_a"] and d["prob_b"] == w["prob_b"]
        print(case, np.max(np.abs(d["raw_prob"] - w["raw"])), np.max(np.abs(d["prob"] - w["prob"])))
        assert np.max(np.abs(d["raw_prob"] - w["raw"])) <= TIGHT and np.max(np.abs(d["prob"] - w["prob"])) <= TIGHT
        assert s == w["segments"]
        assert d["status"][0] == aT.SMO_CONVERGED and len(d["alpha_y"]) == len(d["quiet_idx"]) + len(d["loud_idx"])


def test_a_clip_is_the_same_bytes_alone_first_last_and_across_chunks(gpu_lib):
    clip = onset_ref.burst_clip(0)
    fillers = [onset_ref.burst_clip(10 + k, seconds=1.0 + 0.05 * k) for k in range(38)]
    first = [clip] + fillers + [clip]
    # clip 0 and clip 39 must see one seed: a stream that repeats (Repeating, below)
    args = (onset_ref.FS, 0.02, 0.02, 0.2, 0.4)
    _, alone = aS.silence_removal_batch([clip], *args, random_state=Repeating(7), return_details=True)
    segs, whole = aS.silence_removal_batch(first, *args, random_state=Repeating(7), return_details=True)
    assert same_record(whole[0], alone[0], DETAIL_KEYS) and same_record(whole[39], alone[0], DETAIL_KEYS)
    assert segs[0] == segs[39] and len(segs) == 40
    cut_segs, cut = aS.silence_removal_batch(first, *args, random_state=Repeating(7), return_details=True, chunk_bytes=1 << 20)
    assert cut_segs == segs and all(same_record(a, b, DETAIL_KEYS) for a, b in zip(whole, cut))


def test_int16_float64_and_stereo_follow_the_single_call(gpu_lib):
    mono = onset_ref.burst_clip(1)
    stereo = np.stack([onset_ref.burst_clip(2), onset_ref.burst_clip(3)], axis=1)              # (n, 2) int16
    clips = [mono, mono.astype(np.float64), stereo]
    args = (onset_ref.FS, 0.02, 0.02, 0.2, 0.4)
    np.random.seed(77)
    want = [aS.silence_removal(c, *args, svm_fit="device") for c in clips]
    state = np.random.get_state()[1].copy()
    np.random.seed(77)
    got = aS.silence_removal_batch(clips, *args)
    assert np.array_equal(np.random.get_state()[1], state)          # three draws, as the loop
    for g, w in zip(got, want):
        assert len(w) >= 1 and segments_array(g).shape == segments_array(w).shape
        assert np.allclose(segments_array(g), segments_array(w), rtol=0, atol=1e-9), (g, w)
    assert got[0] == got[1]                                          # the same samples as int16 and as float64


def test_the_batch_needs_no_scikit_learn(gpu_lib, monkeypatch):
    g = load("silence_count_050_050")
    for mod in [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, mod)
    monkeypatch.setitem(sys.modules, "sklearn", None)                       # import sklearn[.x] now raises ImportError
    with pytest.raises(ImportError):
        import sklearn.svm  # noqa: F401
    np.random.seed(int(g["seed"]))
    segs = aS.silence_removal_batch([g["signal"]], 16000, 0.05, 0.05, 0.5, 0.5)
    assert np.allclose(segments_array(segs[0]), g["segments"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("place, chunk_bytes, as_float", [(1, None, False), (2, 500000, False), (0, None, True), (2, 500000, True)])
def test_an_empty_set_names_the_clip(gpu_lib, place, chunk_bytes, as_float):
    """Digital silence: every energy is 0, both limits are 1e-15, every frame is quiet and none is loud.  The whole call refuses the
    clip by its index -- alone in the last chunk of a batch cut into one clip per chunk too, where the first pass over the chunks
    finds it -- and in a batch that travels as float64 as well."""
    silent = np.zeros(3 * onset_ref.FS, dtype=np.int16)
    clips = [onset_ref.burst_clip(0), onset_ref.burst_clip(1)]
    clips.insert(place, silent.astype(np.float64) if as_float else silent)
    with pytest.raises(ValueError, match=r"clip %d: 150 quiet and 0 loud frames: the number of classes has to be greater than one" % place):
        aS.silence_removal_batch(clips, onset_ref.FS, 0.02, 0.02, 0.2, 0.4, chunk_bytes=chunk_bytes)
    good = aS.silence_removal_batch([c for k, c in enumerate(clips) if k != place], onset_ref.FS, 0.02, 0.02, 0.2, 0.4)
    assert all(len(s) >= 1 for s in good)                            # the library serves the next call


def test_more_rows_than_the_solver_serves_names_the_clip(gpu_lib):
    ok, big = onset_ref.burst_clip(0), onset_ref.half_silent_clip()
    with pytest.raises(NotImplementedError, match=r"clip 1: \d+ quiet \+ loud rows.*8192"):
        aS.silence_removal_batch([ok, big], onset_ref.FS, 0.02, 0.01, 0.1, 0.5, random_state=0)      # about 17 000 frames


class Repeating(np.random.RandomState):
    """every draw is the first draw of a fresh RandomState(seed): each clip sees the seed a single call under
    np.random.seed(seed) sees -- for a golden, the seed of the reference's own run"""

    def __init__(self, seed):
        super().__init__(seed)
        self.seed_value = seed

    def randint(self, *a, **k):
        return np.random.RandomState(self.seed_value).randint(*a, **k)


def test_files_are_grouped_by_rate_and_answered_in_path_order(gpu_lib, tmp_path):
    import scipy.io.wavfile as wavfile
    a, b = load("silence_count_050_050"), load("silence_recording1_20s")
    other = onset_ref.burst_clip(4, seconds=4.0)
    paths = [str(tmp_path / n) for n in ("b.wav", "other_8k.wav", "a.wav")]
    wavfile.write(paths[0], 16000, b["signal"])
    wavfile.write(paths[1], 8000, other)
    wavfile.write(paths[2], 16000, a["signal"])
    # the goldens' segments are the reference's under ITS seed (the first draw after np.random.seed(1234)): every file sees that one
    got = aS.silence_removal_files(paths, 0.05, 0.05, 0.5, 0.5, random_state=Repeating(1234))
    assert len(got) == 3
    for g, ref in ((got[0], b), (got[2], a)):
        assert segments_array(g).shape == ref["segments"].shape and np.allclose(segments_array(g), ref["segments"], rtol=0, atol=1e-9), \
            (g, ref["segments"])
    # seeds go by path order, whatever the grouping by rate: the 8 kHz file is the second path and sees the second draw
    np.random.seed(1234)
    by_path = aS.silence_removal_files(paths, 0.05, 0.05, 0.5, 0.5)
    rs = np.random.RandomState(1234)
    rs.randint(np.iinfo('i').max)                                    # the first path's draw
    assert by_path[1] == aS.silence_removal_batch([other], 8000, 0.05, 0.05, 0.5, 0.5, random_state=rs)[0]
    assert by_path[0] == got[0]                                      # the first path saw the first draw both times
    assert by_path == aS.silence_removal_files(paths, 0.05, 0.05, 0.5, 0.5, random_state=np.random.RandomState(1234))
