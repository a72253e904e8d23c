"""silence_removal_batch without a device: the argument errors (each raised before the library is loaded), the seed rule and
where it leaves NumPy's global stream, the ABI of the new entry points, the place of the new kernels in the build, the NumPy
restatement tests/onset_ref.py against the package's host functions, and the margins the GPU tests of
tests/test_onset_batch_gpu.py rely on, asserted here from the oracle's features for every input those tests use."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import onset_ref
import onset_svm_ref
import paa_oracle
from conftest import GOLDEN_DIR, ROOT
from pyaudioanalysis_amd import _build, _ffi, audioSegmentation as aS, audioTrainTest as aT

GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "silence_*.npz")))
NEW_SYMBOLS = ("paa_silence_batch_i16", "paa_silence_batch_f64", "paa_onset_training_sets_f64", "paa_onset_activity_f64")


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def no_device(monkeypatch):
    """the library cannot be loaded: whatever reaches it fails the test"""
    def refuse():
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_ffi, "lib", refuse)


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_a_clip_below_twenty_frames_is_refused_before_the_device(no_device):
    ok, short = np.zeros(16000, dtype=np.int16), np.zeros(19 * 800, dtype=np.int16)        # 20 and 19 frames at 50 / 50 ms
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match=r"clip 1: 19 short-term frames"):
        aS.silence_removal_batch([ok, short, ok], 16000, 0.05, 0.05, smooth_window=0.1)
    assert np.array_equal(np.random.get_state()[1], state)          # no seed was drawn


def test_a_clip_shorter_than_its_smoothing_window_is_refused_before_the_device(no_device):
    clips = [np.zeros(2 * 16000, dtype=np.int16), np.zeros(16000, dtype=np.int16)]          # 40 and 20 frames
    with pytest.raises(ValueError, match=r"clip 1: Input vector needs to be bigger than window size"):
        aS.silence_removal_batch(clips, 16000, 0.05, 0.05, smooth_window=[0.5, 1.5])        # widths 10 and 30
    with pytest.raises(ValueError, match=r"clip 0: Input vector needs to be bigger than window size"):
        aS.silence_removal_batch(clips, 16000, 0.05, 0.05, smooth_window=2.5)               # width 50 for both
    with pytest.raises(ValueError, match="one value per clip"):
        aS.silence_removal_batch(clips, 16000, 0.05, 0.05, weight=[0.5, 0.5, 0.5])


def test_weight_is_clamped_as_in_the_single_call(no_device):
    _, _, frames, widths, weights = aS._onset_plan([16000, 16000, 16000, 16000], 16000, 0.05, 0.05, 0.5, [0.0, 0.3, 1.0, 7.0])
    assert weights.tolist() == [0.01, 0.3, 0.99, 0.99] and frames.tolist() == [20] * 4 and widths.tolist() == [10] * 4


# ---- seeds ------------------------------------------------------------------------------------------------------------------------
def test_none_draws_from_the_global_stream_once_per_clip():
    np.random.seed(31)
    loop = [aT._libsvm_seed(None) for _ in range(4)]
    after_loop = np.random.get_state()[1].copy()
    np.random.seed(31)
    assert aS._batch_seeds(None, 4) == loop
    assert np.array_equal(np.random.get_state()[1], after_loop)


def test_an_int_makes_one_stream_and_a_random_state_is_used_as_is():
    rs = np.random.RandomState(9)
    want = [int(rs.randint(np.iinfo('i').max)) for _ in range(3)]
    state = np.random.get_state()[1].copy()
    assert aS._batch_seeds(9, 3) == want
    mine = np.random.RandomState(9)
    assert aS._batch_seeds(mine, 2) == want[:2] and int(mine.randint(np.iinfo('i').max)) == want[2]
    assert np.array_equal(np.random.get_state()[1], state)          # the global stream is not touched
    assert len(set(want)) == 3


def test_seeds_are_drawn_in_clip_order_before_any_device_work(monkeypatch):
    seen = {}

    def capture(clips, as_i16, fs, window, step, frames, widths, weights, seeds, chunk_bytes, stage_ms):
        seen.setdefault("calls", []).append((as_i16, list(seeds), [c.dtype for c in clips]))
        seen["state"] = np.random.get_state()[1].copy()
        raise RuntimeError("stop before the device")
    monkeypatch.setattr(aS, "_silence_group", capture)
    clips = [np.zeros(16000, dtype=np.int16), np.zeros(16000), np.zeros((16000, 2), dtype=np.int16)]
    np.random.seed(5)
    loop = [aT._libsvm_seed(None) for _ in range(3)]
    after = np.random.get_state()[1].copy()
    np.random.seed(5)
    with pytest.raises(RuntimeError, match="stop before the device"):
        aS.silence_removal_batch(clips, 16000, 0.05, 0.05, smooth_window=0.1)
    assert np.array_equal(seen["state"], after)                      # all three draws were made before the first group ran
    # ONE library call for the whole batch (a refusal after the selection comes before any fit): a mixed batch travels as float64
    assert seen["calls"] == [(False, loop, [np.dtype(np.float64)] * 3)]
    seen.clear()
    with pytest.raises(RuntimeError, match="stop before the device"):
        aS.silence_removal_batch(clips[:1] * 2, 16000, 0.05, 0.05, smooth_window=0.1, random_state=3)
    assert seen["calls"][0][0] is True and seen["calls"][0][2] == [np.dtype(np.int16)] * 2          # all int16: as int16


def test_files_are_checked_before_a_seed_is_drawn(no_device, tmp_path):
    import scipy.io.wavfile as wavfile
    paths = [str(tmp_path / n) for n in ("ok.wav", "ok_8k.wav", "short.wav")]
    wavfile.write(paths[0], 16000, np.zeros(16000, dtype=np.int16))
    wavfile.write(paths[1], 8000, np.zeros(8000, dtype=np.int16))
    wavfile.write(paths[2], 16000, np.zeros(19 * 800, dtype=np.int16))           # 19 frames at 50 / 50 ms
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match=r"clip 2: 19 short-term frames"):        # named by its place among the paths
        aS.silence_removal_files(paths, 0.05, 0.05, smooth_window=0.1)
    with pytest.raises(ValueError, match=r"clip 1: Input vector needs to be bigger than window size"):
        aS.silence_removal_files(paths[:2], 0.05, 0.05, smooth_window=[0.5, 1.5])
    with pytest.raises(ValueError, match=r"file 1 .*cannot be read"):
        aS.silence_removal_files([paths[0], str(tmp_path / "missing.wav")], 0.05, 0.05)
    assert np.array_equal(np.random.get_state()[1], state)          # no seed was drawn


# ---- ABI and build ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    handle = ctypes.CDLL(_build.build())
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _ffi.EXPORTED_SYMBOLS
        assert hasattr(handle, name), name
    i16, f64 = _ffi._SIGNATURES["paa_silence_batch_i16"][1], _ffi._SIGNATURES["paa_silence_batch_f64"][1]
    assert i16[0] is _ffi.c_i16p and f64[0] is _ffi.c_f64p and i16[1:] == f64[1:] and len(i16) == 32


def test_the_kernels_live_in_the_smo_unit():
    unit = open(os.path.join(_build.CSRC, "family_smo.hip")).read()
    assert '#include "kernels_onset.hpp"' in unit
    assert len(_build.SOURCES) == 18 and "family_smo.hip" in _build.SOURCES and "family_smo.hip" not in _build.UNIT_FLAGS
    kernels = open(os.path.join(_build.CSRC, "kernels_onset.hpp")).read()
    for name in ("onset_select_kernel", "onset_gather_kernel", "onset_proba_kernel", "onset_threshold_kernel"):
        assert "void %s(" % name in kernels
    assert "atomicAdd(&hist" in kernels and not re.search(r"atomicAdd\([^)]*double", kernels)       # integer counts only
    assert '#include "lib_onset.hpp"' in open(os.path.join(_build.CSRC, "paa_lib.hip")).read()


# ---- the restatement against the package's host functions ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", onset_ref.STAGE1_KINDS)
def test_restated_selection_equals_energy_extremes(kind):
    for T in onset_ref.STAGE1_FRAMES:
        st = onset_ref.stage1_case(kind, T)
        ref = onset_ref.training_sets(st)
        quiet, loud = aS._energy_extremes(st)
        assert np.array_equal(quiet, st[:, ref["quiet_idx"]]) and np.array_equal(loud, st[:, ref["loud_idx"]]), (kind, T)
        assert np.array_equal(ref["features"], np.vstack([quiet.T, loud.T]))
        ranked = np.sort(st[1])
        tenth = T // 10
        np_limits = (ranked[:tenth].mean() + 1e-15, ranked[-tenth:-1].mean() + 1e-15)
        for mine, theirs in zip((ref["quiet_limit"], ref["loud_limit"]), np_limits):
            if kind in onset_ref.EXACT_KINDS:
                assert mine == theirs
            else:
                assert abs(mine - theirs) <= onset_ref.limit_bound(tenth) * theirs
        if len(ref["features"]) >= 3:
            feats = ref["features"]
            scale = np.sqrt(feats.var(axis=0))
            scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
            assert np.array_equal(ref["mean"], feats.mean(axis=0)) and np.array_equal(ref["scale"], scale)       # NumPy's bits


def test_stage1_kinds_are_what_they_claim():
    sets = {T: onset_ref.training_sets(onset_ref.stage1_case("overlap", T)) for T in onset_ref.STAGE1_FRAMES}
    for T, r in sets.items():
        assert len(r["quiet_idx"]) == T and len(r["loud_idx"]) == 1 and r["loud_idx"][0] in r["quiet_idx"]      # a frame in both sets
    for T in onset_ref.STAGE1_FRAMES:
        r = onset_ref.training_sets(onset_ref.stage1_case("all_equal", T))
        assert len(r["quiet_idx"]) == T and len(r["loud_idx"]) == 0
        e = np.sort(onset_ref.stage1_case("tie_run", T)[1])
        assert e[T // 10 - 1] == e[T // 10] == 0.2 and e[0] < 0.2                    # the run straddles rank tenth
        z = onset_ref.stage1_case("zeros_and_noise", T)[1]
        assert (z == 0).sum() >= 1 and (z > 0).sum() >= 1
        d = onset_ref.stage1_case("dyadic", T)[1] * 2.0 ** 20
        assert np.array_equal(d, np.round(d))
    const = np.ascontiguousarray(onset_ref.stage1_case("random", 117))
    const[5] = 3.25
    assert onset_ref.training_sets(const)["scale"][5] == 1.0 and onset_ref.training_sets(const)["mean"][5] == 3.25


def test_restated_smoothing_and_threshold_equal_the_host_functions():
    rng = np.random.default_rng(3)
    for n, width in ((20, 2), (20, 3), (29, 29), (117, 10), (117, 11), (400, 20), (293, 50)):
        v = rng.uniform(0.0, 1.0, n)
        got, ref = onset_ref.smooth(v, width), aS.smooth_moving_avg(v, width)
        assert (got is v and ref is v) if width < 3 else np.max(np.abs(got - ref)) <= 1e-14
        for weight in (0.01, 0.5, 0.99):
            assert abs(onset_ref.threshold(ref, weight) - aS._onset_threshold(ref, weight)) <= 1e-14
    with pytest.raises(ValueError):
        onset_ref.smooth(np.zeros(5), 6)


def test_stage45_cases_keep_their_margins():
    for T, width, weight in onset_ref.STAGE45_CASES:
        _, _, ref = onset_ref.stage45_case(T, width, weight)
        assert ref["exit_margin"] > onset_svm_ref.MARGIN_MIN and ref["thr_margin"] > 1e-6
        assert 0 < len(ref["active"]) < T
    widths = [c[1] for c in onset_ref.STAGE45_CASES]
    assert 2 in widths and 3 in widths and any(w % 2 == 0 and w > 3 for w in widths) and any(w % 2 == 1 and w > 3 for w in widths)
    assert any(c[0] == c[1] for c in onset_ref.STAGE45_CASES) and {c[2] for c in onset_ref.STAGE45_CASES} == {0.01, 0.5, 0.99}


# ---- the margins of the whole-call inputs, from the oracle's features --------------------------------------------------------------
def whole_call_inputs():
    """(name, signal, fs, st_win, st_step, smooth_window, weight, seed) of every clip the whole-call GPU tests compare
    against a reference: the four goldens and the synthetic clips of the loop comparison"""
    out = []
    for path in GOLDENS:
        g = load(path)
        out.append((os.path.basename(path), g["signal"], int(g["fs"]), float(g["st_win"]), float(g["st_step"]),
                    float(g["smooth_window"]), float(g["weight"]), int(g["seed"])))
    for k in range(3):
        out.append(("burst_%d" % k, onset_ref.burst_clip(k), onset_ref.FS, 0.02, 0.02, 0.2, 0.4, 1234))
    stereo = onset_ref.burst_clip(3) / 2 + onset_ref.burst_clip(2) / 2          # stereo_to_mono of the two-channel clip
    out.append(("stereo_2_3", stereo, onset_ref.FS, 0.02, 0.02, 0.2, 0.4, 77))
    return out


@pytest.mark.parametrize("case", whole_call_inputs(), ids=lambda c: c[0])
def test_selection_margins_of_the_whole_call_inputs(case):
    name, signal, fs, st_win, st_step = case[:5]
    st, _ = paa_oracle.feature_extraction(signal, fs, int(st_win * fs), int(st_step * fs))
    ref = onset_ref.training_sets(st)
    assert st.shape[1] >= 20 and len(ref["quiet_idx"]) >= 1 and len(ref["loud_idx"]) >= 1
    assert onset_ref.selection_margin_ok(st[1], (ref["quiet_limit"], ref["loud_limit"])), name


@pytest.mark.parametrize("case", whole_call_inputs(), ids=lambda c: c[0])
def test_threshold_margins_of_the_whole_call_inputs(case):
    pytest.importorskip("sklearn.svm")
    name, signal, fs, st_win, st_step, smooth_window, weight, seed = case
    st, _ = paa_oracle.feature_extraction(signal, fs, int(st_win * fs), int(st_step * fs))
    quiet, loud = aS._energy_extremes(st)
    np.random.seed(seed)
    svm, mean, scale = aS._train_onset_svm(quiet.T, loud.T)
    w = (np.asarray(svm.dual_coef_).reshape(-1)[:, None] * svm.support_vectors_).sum(axis=0)
    model = (w, float(svm.intercept_[0]), float(svm.probA_[0]), float(svm.probB_[0]), mean, scale)
    ref = onset_ref.activity(st, model, int(smooth_window / st_step), weight)
    assert ref["thr_margin"] > 1e-6, (name, ref["thr_margin"])
