"""CPU checks of the HMM segmentation path (audioSegmentation.GaussianHmm, train_hmm_compute_statistics, load_hmm / save_hmm,
hmm_segmentation): the NumPy restatement (tests/hmm_ref.py) against the stored outputs and, where the reference tree is
present, against the live reference's train_hmm_compute_statistics; the goldens' format; the model-file loader without
hmmlearn; argument validation that needs no device; no CPU fallback."""
import ctypes as C
import os
import pickle
import sys
import types

import numpy as np
import pytest

import hmm_ref
from conftest import GOLDEN_DIR, golden_files, golden_id
from pyaudioanalysis_amd import _ffi, audioSegmentation as aS

MIN_MARGIN = 1e-3


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _named(name):
    return _load(os.path.join(GOLDEN_DIR, name + ".npz"))


def _by_case(*cases):
    return [f for f in golden_files("hmm") if str(np.load(f, allow_pickle=False)["case"]) in cases]


def test_hmm_goldens_are_plain_arrays():
    files = golden_files("hmm")
    assert len(files) >= 10
    largest = max(os.path.getsize(os.path.join(GOLDEN_DIR, f)) for f in os.listdir(GOLDEN_DIR) if not f.startswith("hmm_"))
    cases = set()
    for f in files:
        assert os.path.getsize(f) <= largest, f
        with np.load(f, allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files)
            cases.add(str(z["case"]))
    assert cases == {"radio", "radio_concat", "signal_tail", "train", "ties", "synth", "edges"}


@pytest.mark.parametrize("path", _by_case("radio", "radio_concat", "train", "ties"), ids=golden_id)
def test_restatement_matches_stored_outputs(path):
    g = _load(path)
    X = g["mid"].T
    assert np.array_equal(hmm_ref.log_likelihood(X, g["means"], g["covars"]), g["want_loglik"])
    lp, st, mg = hmm_ref.decode(g["startprob"], g["transmat"], g["means"], g["covars"], X)
    assert np.array_equal(st, g["want_states"]) and np.array_equal(lp, g["want_logprob"]) and np.array_equal(mg, g["want_margins"])
    if str(g["case"]) != "ties":
        assert mg.min() >= MIN_MARGIN
    else:
        tied = mg == 0
        assert tied[-1] or tied[:-1].any()
        assert np.count_nonzero(tied) > 50 and (g["startprob"] == 0).any() and (g["transmat"] == 0).any()


def test_shipped_model_golden():
    g = _named("hmm_radio_sm_concat")
    assert g["means"].shape == (2, 136) and [str(c) for c in g["class_names"]] == ["music", "speech"]
    assert float(g["mid_window"]) == 1.0 and float(g["mid_step"]) == 1.0


def test_synthetic_cases_restate(monkeypatch):
    g = _named("hmm_synth")
    assert g["min_margin"].min() >= MIN_MARGIN and float(g["ragged_min_margin"]) >= MIN_MARGIN
    assert {1, 2, 8, 32} <= set(g["rows"][:, 0].tolist()) and {1, 136, 256} <= set(g["rows"][:, 1].tolist())
    assert {1, 2, 255, 256, 257, 775, 36000} <= set(g["rows"][:, 3].tolist())
    pos = 0
    for (K, D, seed, T), want_lp in zip(g["rows"], g["want_logprob"]):
        if T <= 800 and D <= 136:                 # the long and wide ones are the golden script's job
            model = hmm_ref.synthetic_model(int(K), int(D), int(seed), zeros=True)
            lp, st, _ = hmm_ref.decode(*model, hmm_ref.synthetic_sequence(model, int(T), int(seed) + 1000))
            assert np.array_equal(st, g["want_states"][pos:pos + T]) and lp[0] == want_lp
        pos += int(T)
    assert pos == g["want_states"].shape[0]


def test_training_statistics_restatement_and_live_reference():
    import load_reference
    cases = [(_named(n)["mid"], _named(n)["flags"], _named(n)) for n in ("hmm_train_diar_1s", "hmm_train_diar_01s")]
    for mid, flags, g in cases:
        out = hmm_ref.train_statistics(mid, flags)
        for a, key in zip(out, ("startprob", "transmat", "means", "covars")):
            assert np.array_equal(a, g[key], equal_nan=True), key
        assert (g["transmat"] == 0).any()
    e = _named("hmm_train_edges")
    for name in ("long_labels", "single_window", "never_left"):
        out = hmm_ref.train_statistics(e["feats"], e[name + "_labels"])
        for a, key in zip(out, ("priors", "transmat", "means", "covars")):
            assert np.array_equal(a, e[name + "_" + key], equal_nan=True), (name, key)
    if not load_reference.reference_available():
        return
    import warnings
    ref_seg = load_reference.load_segmentation()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for mid, flags, g in cases:
            out = ref_seg.train_hmm_compute_statistics(mid, flags)
            for a, key in zip(out, ("startprob", "transmat", "means", "covars")):
                assert np.array_equal(a, g[key], equal_nan=True), key


def _reference_format_file(path, model_fields, names, win, step):
    """A model file as the reference writes it, pickled from a throw-away hmmlearn.hmm module object."""
    mods = {n: sys.modules.get(n) for n in ("hmmlearn", "hmmlearn.hmm", "hmmlearn.base")}
    try:
        for n in mods:
            sys.modules[n] = types.ModuleType(n)
        hmm_cls = type("GaussianHMM", (), {"__module__": "hmmlearn.hmm"})
        mon_cls = type("ConvergenceMonitor", (), {"__module__": "hmmlearn.base"})
        sys.modules["hmmlearn.hmm"].GaussianHMM = hmm_cls
        sys.modules["hmmlearn.base"].ConvergenceMonitor = mon_cls
        obj, mon = hmm_cls(), mon_cls()
        import collections
        mon.__dict__.update({"tol": 0.01, "n_iter": 10, "verbose": False, "history": collections.deque(maxlen=2), "iter": 0})
        obj.__dict__.update({"n_components": len(model_fields[0]), "covariance_type": "diag", "monitor_": mon,
                             "startprob_": model_fields[0], "transmat_": model_fields[1], "means_": model_fields[2],
                             "_covars_": model_fields[3]})
        with open(path, "wb") as f:
            for o in (obj, names, win, step):
                pickle.dump(o, f, protocol=pickle.HIGHEST_PROTOCOL)
    finally:
        for n, m in mods.items():
            if m is None:
                del sys.modules[n]
            else:
                sys.modules[n] = m


def test_load_hmm_reads_reference_files_without_hmmlearn(tmp_path):
    g = _named("hmm_radio_sm_concat")
    fields = (g["startprob"], g["transmat"], g["means"], g["covars"])
    path = str(tmp_path / "ref_model")
    _reference_format_file(path, fields, ["music", "speech"], 1.0, 1.0)
    assert "hmmlearn" not in sys.modules or sys.modules["hmmlearn"] is not None
    hmm, names, win, step = aS.load_hmm(path)
    assert isinstance(hmm, aS.GaussianHmm) and hmm.n_components == 2 and hmm.covariance_type == "diag"
    for a, b in zip((hmm.startprob_, hmm.transmat_, hmm.means_, hmm.covars_), fields):
        assert np.array_equal(a, b)
    assert names == ["music", "speech"] and win == 1.0 and step == 1.0
    # our own files round-trip, and a stand-in with the four attributes is accepted wherever a model is
    ours = str(tmp_path / "our_model")
    aS.save_hmm(ours, hmm, names, win, step)
    again = aS.load_hmm(ours)
    assert np.array_equal(again[0].means_, hmm.means_) and again[1:] == (names, win, step)
    stand_in = types.SimpleNamespace(startprob_=fields[0], transmat_=fields[1], means_=fields[2], _covars_=fields[3])
    assert np.array_equal(aS.as_gaussian_hmm(stand_in).covars_, fields[3])


def test_load_hmm_reads_the_shipped_model():
    import load_reference
    if not load_reference.reference_available():
        pytest.skip("reference tree not present")
    path = os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", "hmmRadioSM")
    hmm, names, win, step = aS.load_hmm(path)
    g = _named("hmm_radio_sm_concat")
    assert hmm.n_components == 2 and hmm.n_features == 136 and names == ["music", "speech"] and win == 1.0 and step == 1.0
    assert np.array_equal(hmm.means_, g["means"]) and np.array_equal(hmm.covars_, g["covars"])


def test_load_hmm_refuses_other_globals(tmp_path):
    path = str(tmp_path / "bad")
    with open(path, "wb") as f:
        for o in (os.path.join, ["a"], 1.0, 1.0):
            pickle.dump(o, f)
    with pytest.raises(pickle.UnpicklingError):
        aS.load_hmm(path)


def test_python_argument_validation():
    with pytest.raises(IndexError):
        aS.train_hmm_compute_statistics(np.zeros((3, 6)), np.array([0, 2, 2, 0, 0, 2]))
    with pytest.raises(ValueError):
        aS.GaussianHmm([0.5, 0.5], np.eye(3), np.zeros((2, 4)), np.ones((2, 4)))
    hmm = aS.GaussianHmm([0.5, 0.5], np.eye(2), np.zeros((2, 4)), np.ones((2, 4)))
    with pytest.raises(ValueError):
        hmm.decode(np.zeros((5, 3)))
    with pytest.raises(ValueError):
        hmm._offsets([2, 0, 3], 5)
    for name in ("train_hmm_from_file", "train_hmm_from_directory", "hmm_segmentation", "hmm_segmentation_signal", "load_hmm"):
        assert callable(getattr(aS, name))


def test_c_abi_rejects_bad_models_and_arguments():
    """PAA_ERR_ARG before any device work, so this holds with and without a GPU."""
    lib = _ffi.lib()
    h = C.c_void_p()
    K, D = 3, 4
    start, trans, means, cov = np.full(K, 1 / 3.0), np.full((K, K), 1 / 3.0), np.zeros((K, D)), np.ones((K, D))

    def create(s=start, t=trans, m=means, c=cov, k=K, d=D, out=True):
        p = [_ffi.as_f64p(np.ascontiguousarray(a)) if a is not None else None for a in (s, t, m, c)]
        return lib.paa_hmm_create(*p, k, d, C.byref(h) if out else None)
    nan_row = trans.copy()
    nan_row[1] = np.nan
    zero_cov = cov.copy()
    zero_cov[2, 1] = 0
    for kw in ({"k": 0}, {"k": 33}, {"d": 0}, {"d": 257}, {"s": None}, {"out": False}, {"t": nan_row}, {"c": zero_cov},
               {"c": cov * np.inf}, {"s": np.array([0.5, 0.6, -0.1])}, {"s": start * (1 + 1e-6)}, {"m": means + np.nan}):
        assert create(**kw) == _ffi.ERR_ARG, kw
    assert lib.paa_hmm_num_states(None) == _ffi.ERR_ARG and lib.paa_hmm_destroy(None) == _ffi.PAA_OK
    x = np.zeros(8)
    o = np.array([0, 1], dtype=np.int64)
    s = np.zeros(2, dtype=np.int32)
    assert lib.paa_hmm_decode_f64(None, _ffi.as_f64p(x), 4, 1, 1, _ffi.as_i64p(o), 1, s.ctypes.data_as(_ffi.c_i32p),
                                  _ffi.as_f64p(x)) == _ffi.ERR_ARG
    assert lib.paa_hmm_dev_decode_f64(None, None, 4, 1, 1, None, 1, None, None) == _ffi.ERR_ARG
    assert lib.paa_hmm_dev_loglik_f64(None, None, 4, 1, 1, None) == _ffi.ERR_ARG
    lab = np.array([0, 5], dtype=np.int32)
    outs = [_ffi.as_f64p(np.zeros(16)) for _ in range(4)]
    assert lib.paa_hmm_train_stats_f64(_ffi.as_f64p(x), 4, 2, 2, lab.ctypes.data_as(_ffi.c_i32p), 2, *outs) == _ffi.ERR_ARG
    assert lib.paa_hmm_train_stats_f64(_ffi.as_f64p(x), 4, 2, 2, s.ctypes.data_as(_ffi.c_i32p), 33, *outs) == _ffi.ERR_ARG
    assert lib.paa_hmm_dev_train_stats_f64(None, 4, 2, 2, s.ctypes.data_as(_ffi.c_i32p), 2, *outs) == _ffi.ERR_ARG


def test_no_cpu_fallback():
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present")
    g = _named("hmm_ties")
    hmm = aS.GaussianHmm(g["startprob"], g["transmat"], g["means"], g["covars"])
    with pytest.raises(_ffi.HipLibraryError):
        hmm.predict(g["mid"].T)
    with pytest.raises(_ffi.HipLibraryError):
        aS.train_hmm_compute_statistics(g["mid"], np.arange(g["mid"].shape[1]) % 2)
    with pytest.raises(_ffi.HipLibraryError):
        aS.hmm_segmentation_signal(np.zeros(32000, dtype=np.int16), 16000, hmm, ["a"] * 5, 1.0, 1.0)
