"""GPU tests of the Gaussian HMM segmenter (kernels_hmm.hpp): emission matrix, Viterbi (one wave per sequence and by blocks),
training statistics and the audioSegmentation drop-ins, against the hmm_* goldens (the unmodified reference's mid-term
matrices and training statistics, scripts/make_hmm_golden.py) and the NumPy restatement (tests/hmm_ref.py).

Gates: emission matrix, logprob and the statistics 1e-9 relative to max(|ref|, 1); counts, priors and transition rows exact;
states identical at every step.  The latter is asked only of inputs whose every decision has a restatement margin of at
least 1e-3 nats (asserted from the stored margins first); in hmm_ties exactly tied steps must give the lowest index.
Observed maxima (MI355X): see DESIGN §4 K10."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

import hmm_ref
from conftest import GOLDEN_DIR, golden_files, golden_id
from pyaudioanalysis_amd import _ffi, audioSegmentation as aS

pytestmark = pytest.mark.gpu
GATE = 1e-9
MIN_MARGIN = 1e-3
BLOCK = 256


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _named(name):
    return _load(os.path.join(GOLDEN_DIR, name + ".npz"))


def _by_case(*cases):
    return [f for f in golden_files("hmm") if str(np.load(f, allow_pickle=False)["case"]) in cases]


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if want.size else 0.0


def _model(g):
    return aS.GaussianHmm(g["startprob"], g["transmat"], g["means"], g["covars"])


def _device_run(hmm, X, lengths=None, block_rows=None):
    """(loglik, logprob per sequence, states) of X [n_windows][n_dims] through the device-buffer entry points."""
    F = np.ascontiguousarray(X.T)
    d = _ffi.DeviceBuffer.from_host(F)
    try:
        B = hmm.log_likelihood_device(d, F.shape[1], F.shape[1])
        offsets = None if lengths is None else np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
        lp, st = hmm.predict_device(d, F.shape[1], F.shape[1], offsets, block_rows)
    finally:
        d.free()
    return B, lp, st


@pytest.mark.parametrize("path", _by_case("radio", "radio_concat", "train", "ties"), ids=golden_id)
def test_emission_and_decode_match_restatement(gpu_lib, path):
    g = _load(path)
    ties = str(g["case"]) == "ties"
    m = g["want_margins"]
    if not ties:
        assert m.min() >= MIN_MARGIN
    hmm = _model(g)
    X = g["mid"].T
    B, lp, st = _device_run(hmm, X)
    e_B, e_lp = _rel(B, g["want_loglik"]), _rel(lp, g["want_logprob"])
    print("%s: %d windows, loglik err %.3g, logprob err %.3g, min margin %.3g" % (golden_id(path), X.shape[0], e_B, e_lp, m.min()))
    assert e_B <= GATE and e_lp <= GATE
    assert np.array_equal(st, g["want_states"])           # every step, tied ones included (lowest index)
    if ties:
        assert np.count_nonzero(m == 0) > 50 and m[m > 0].min() >= MIN_MARGIN
    # host-matrix entry points: hmmlearn's calling convention
    lp2, st2 = hmm.decode(X)
    assert np.array_equal(st2, st) and lp2 == lp[0] and np.array_equal(hmm.predict(X), st)


def test_synthetic_models_every_length(gpu_lib):
    g = _named("hmm_synth")
    pos, worst_B, worst_lp = 0, 0.0, 0.0
    for (K, D, seed, T), want_lp, margin in zip(g["rows"], g["want_logprob"], g["min_margin"]):
        assert margin >= MIN_MARGIN
        model = hmm_ref.synthetic_model(int(K), int(D), int(seed), zeros=True)
        X = hmm_ref.synthetic_sequence(model, int(T), int(seed) + 1000)
        hmm = aS.GaussianHmm(*model)
        B, lp, st = _device_run(hmm, X)
        want = g["want_states"][pos:pos + T]
        pos += int(T)
        e_B, e_lp = _rel(B, hmm_ref.log_likelihood(X, model[2], model[3])), _rel(lp, np.array([want_lp]))
        worst_B, worst_lp = max(worst_B, e_B), max(worst_lp, e_lp)
        print("K %d D %d T %d: loglik err %.3g, logprob err %.3g, min margin %.3g" % (K, D, T, e_B, e_lp, margin))
        assert e_B <= GATE and e_lp <= GATE, (K, D, T)
        assert np.array_equal(st, want), (K, D, T, int(np.count_nonzero(st != want)))
        if T > BLOCK:         # the same sequence through the one-wave path: same states, logprob to rounding
            _, lp1, st1 = _device_run(hmm, X, block_rows=int(T))
            assert np.array_equal(st1, want) and _rel(lp1, lp) <= GATE, (K, D, T)
    print("worst: loglik %.3g, logprob %.3g" % (worst_B, worst_lp))


def test_ragged_batch(gpu_lib):
    g = _named("hmm_synth")
    K, D, seed, n_seq, longest = (int(v) for v in g["ragged"])
    assert float(g["ragged_min_margin"]) >= MIN_MARGIN
    lengths = g["ragged_lengths"]
    model = hmm_ref.synthetic_model(K, D, seed, zeros=True)
    X = hmm_ref.synthetic_sequence(model, int(lengths.sum()), seed + 1000)
    hmm = aS.GaussianHmm(*model)
    _, lp, st = _device_run(hmm, X, lengths)
    assert np.array_equal(st, g["ragged_states"]) and _rel(lp, g["ragged_logprob"]) <= GATE
    lp_h, st_h = hmm.decode_sequences(X, lengths)
    assert np.array_equal(st_h, st) and np.array_equal(lp_h, lp)
    # sequence by sequence through the same entry point: bit-identical where the code path is the same (one segment),
    # states equal and logprob at the gate otherwise -- the path is the same here too (same cuts), so all are identical
    starts = np.concatenate(([0], np.cumsum(lengths)))
    for q in list(range(0, n_seq, 37)) + [1]:
        _, lp1, st1 = _device_run(hmm, X[starts[q]:starts[q + 1]])
        assert np.array_equal(st1, st[starts[q]:starts[q + 1]]), q
        if lengths[q] <= BLOCK:
            assert lp1[0] == lp[q], q
        else:
            assert _rel(lp1, lp[q:q + 1]) <= GATE, q


def test_training_statistics_match_reference(gpu_lib):
    for name in ("hmm_train_diar_1s", "hmm_train_diar_01s"):
        g = _named(name)
        pri, trans, means, cov = aS.train_hmm_compute_statistics(g["mid"], g["flags"])
        assert np.array_equal(pri, g["startprob"]) and np.array_equal(trans, g["transmat"], equal_nan=True)
        e_m, e_c = _rel(means, g["means"]), _rel(cov, g["covars"])
        print("%s: means err %.3g, std err %.3g" % (name, e_m, e_c))
        assert e_m <= GATE and e_c <= GATE
        d = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(g["mid"]))
        out = aS.train_hmm_compute_statistics_device(d, g["mid"].shape[0], g["mid"].shape[1], g["mid"].shape[1], g["flags"])
        d.free()
        for a, b in zip(out, (pri, trans, means, cov)):
            assert np.array_equal(a, b, equal_nan=True)


def test_training_edge_cases(gpu_lib):
    g = _named("hmm_train_edges")
    for name in ("long_labels", "single_window", "never_left"):
        with contextlib.redirect_stdout(io.StringIO()) as printed:
            pri, trans, means, cov = aS.train_hmm_compute_statistics(g["feats"], g[name + "_labels"])
        assert ("trainHMM warning" in printed.getvalue()) == (name == "long_labels")
        assert np.array_equal(pri, g[name + "_priors"])
        assert np.array_equal(np.isnan(trans), np.isnan(g[name + "_transmat"]))
        assert np.array_equal(trans, g[name + "_transmat"], equal_nan=True)
        assert _rel(means, g[name + "_means"]) <= GATE and _rel(cov, g[name + "_covars"]) <= GATE
        if name == "single_window":
            assert np.all(cov[2] == 0)
        if name != "long_labels":           # std 0 / a NaN row: refused at model creation
            with pytest.raises(ValueError):
                aS.GaussianHmm(pri, trans, means, cov).predict(g["feats"].T)
    with pytest.raises(IndexError):
        aS.train_hmm_compute_statistics(g["feats"], np.array([0, 2] * 25))
    # the device is usable afterwards
    g2 = _named("hmm_ties")
    assert np.array_equal(_model(g2).predict(g2["mid"].T), g2["want_states"])


def _signal(g, name):
    sig = g["signal"]
    if "signal_length" in g and int(g["signal_length"]) > sig.shape[0]:
        sig = np.concatenate([sig, _named(name + "_tail")["signal"]])
    return sig


@pytest.mark.parametrize("clip", ["speech_music_sample", "diarizationExample", "count2"])
def test_hmm_segmentation_end_to_end(gpu_lib, tmp_path, clip):
    import scipy.io.wavfile as wavfile
    name = "hmm_radio_sm_" + clip
    g = _named(name)
    wav, model = str(tmp_path / "x.wav"), str(tmp_path / "hmm")
    wavfile.write(wav, int(g["fs"]), _signal(g, name))
    aS.save_hmm(model, _model(g), [str(c) for c in g["class_names"]], float(g["mid_window"]), float(g["mid_step"]))
    labels, names, acc, cm = aS.hmm_segmentation(wav, model)
    assert names == [str(c) for c in g["class_names"]]
    assert np.array_equal(labels, g["want_states"])           # the restatement on the live reference's mid-term matrix


def test_train_hmm_from_file(gpu_lib, tmp_path):
    import scipy.io.wavfile as wavfile
    g = _named("hmm_train_diar_1s")
    src = str(g["signal_from"])
    wav, gt, model = str(tmp_path / "d.wav"), str(tmp_path / "d.segments"), str(tmp_path / "hmm")
    wavfile.write(wav, int(g["fs"]), _signal(_named(src), src))
    with open(gt, "w") as f:
        for (s, e), lab in zip(g["gt_segments"], g["gt_labels"]):
            f.write("%r\t%r\t%s\n" % (float(s), float(e), lab))
    hmm, names = aS.train_hmm_from_file(wav, gt, model, 1.0, 1.0)
    # class names come from a set: map ours onto the golden's order
    order = [names.index(str(c)) for c in g["class_names"]]
    assert sorted(order) == list(range(len(names)))
    assert np.allclose(hmm.startprob_[order], g["startprob"], rtol=0, atol=0)
    assert np.array_equal(hmm.transmat_[np.ix_(order, order)], g["transmat"], equal_nan=True)
    import paa_oracle as O
    for ours, ref in ((hmm.means_[order], g["means"]), (hmm.covars_[order], g["covars"])):
        nbad, _ = O.mixed_tolerance_violations(ours, ref)       # the mid-term parity gate
        assert nbad == 0
    h2, names2, win, step = aS.load_hmm(model)
    assert names2 == names and win == 1.0 and step == 1.0 and np.array_equal(h2.means_, hmm.means_)


def test_argument_errors_leave_the_device_usable(gpu_lib):
    lib = gpu_lib
    g = _named("hmm_ties")
    hmm = _model(g)
    K, D = hmm.n_components, hmm.n_features
    h = C.c_void_p()

    def create(start=hmm.startprob_, trans=hmm.transmat_, means=hmm.means_, covars=hmm.covars_, k=K, d=D):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (start, trans, means, covars)]
        return lib.paa_hmm_create(*[_ffi.as_f64p(a) for a in arrs], k, d, C.byref(h))
    bad_cov, nan_mean, neg, off = hmm.covars_.copy(), hmm.means_.copy(), hmm.startprob_.copy(), hmm.transmat_.copy()
    bad_cov[1, 0] = 0.0
    nan_mean[0, 1] = np.nan
    neg[0], neg[1] = -0.25, 0.75
    off[2, 2] += 1e-6
    nan_row = hmm.transmat_.copy()
    nan_row[4] = np.nan
    for kw in ({"k": 0}, {"k": 33}, {"d": 0}, {"d": 257}, {"covars": bad_cov}, {"covars": -hmm.covars_}, {"means": nan_mean},
               {"start": neg}, {"trans": off}, {"trans": nan_row}, {"start": hmm.startprob_ * 0.5}):
        assert create(**kw) == _ffi.ERR_ARG, kw
    X = np.ascontiguousarray(g["mid"])
    n = X.shape[1]
    d = _ffi.DeviceBuffer.from_host(X)
    d_s, d_l = _ffi.DeviceBuffer(4 * n), _ffi.DeviceBuffer(16)

    def dev(offsets, n_seq, n_dims=D, ld=n, n_vec=n):
        o = np.array(offsets, dtype=np.int64)
        return lib.paa_hmm_dev_decode_f64(hmm.handle, d.ptr, n_dims, ld, n_vec, _ffi.as_i64p(o), n_seq, d_s.ptr, d_l.ptr)
    assert dev([0, 5, 5, n], 3) == _ffi.ERR_ARG               # an empty sequence
    assert dev([0, n - 1], 1) == _ffi.ERR_ARG                 # offsets stop short
    assert dev([1, n], 1) == _ffi.ERR_ARG
    assert dev([0, n], 1, n_dims=D + 1) == _ffi.ERR_ARG
    assert dev([0, n], 1, ld=n - 1) == _ffi.ERR_ARG
    assert dev([0, n], 0) == _ffi.ERR_ARG
    assert lib.paa_hmm_dev_loglik_f64(hmm.handle, d.ptr, D, n, 0, d_s.ptr) == _ffi.ERR_ARG
    lab = np.zeros(n, dtype=np.int32)
    lab[3] = 7
    out = [np.zeros(64) for _ in range(4)]
    assert lib.paa_hmm_dev_train_stats_f64(d.ptr, D, n, n, lab.ctypes.data_as(_ffi.c_i32p), 2, *[_ffi.as_f64p(a) for a in out]) \
        == _ffi.ERR_ARG
    assert dev([0, n], 1) == _ffi.PAA_OK                      # and a valid call right after
    st = d_s.to_host(np.int32, n)
    assert np.array_equal(st, g["want_states"])
    for b in (d, d_s, d_l):
        b.free()
