"""GPU speaker diarization (kernels_diar.hpp, audioSegmentation.diarize_features / speaker_diarization_signal) against the
goldens of scripts/make_diar_golden.py (SciPy / scikit-learn stage outputs from stored initial centres) and against the NumPy
restatement tests/diar_ref.py.  Numbers are held to 1e-9 relative to max(|ref|, 1); decisions (kept dimensions, labels,
n_iter, imax, HMM states, filtered labels) must be IDENTICAL wherever the stored margin of the decision is at least a floor:
a relative gap of 1e-6 for the distance-based ones (a thousand times the gate on the compared quantities), 1e-3 nats for the
HMM.  The floors are asserted from the golden first, and the real-audio goldens may not exclude anything."""
import ctypes as C
import os

import numpy as np
import pytest

import diar_ref
import svc_libsvm
from conftest import golden_files, golden_id, load_golden
from pyaudioanalysis_amd import _ffi
from pyaudioanalysis_amd import audioSegmentation as aS
from pyaudioanalysis_amd import audioTrainTest

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
DIST_FLOOR = 1e-6
HMM_FLOOR = 1e-3
REAL = ("diar_example", "diar_example_2s", "diar_example2")
GOLDENS = golden_files("diar")


def assert_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    err = np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1.0)
    print("%s: max err %.3g" % (what, err))
    assert err <= TIGHT, (what, err)


def init_of(g):
    return {int(k): g["k%d_init" % k] for k in g["ks"]}


def test_goldens_present():
    assert sorted(golden_id(p) for p in GOLDENS) == ["diar_const", "diar_example", "diar_example2", "diar_example_2s", "diar_synth"]


@pytest.mark.parametrize("path", GOLDENS, ids=golden_id)
def test_cluster_stages_match_golden(gpu_lib, path):
    g = load_golden(path)
    name = golden_id(path)
    M = g["M"]
    d_m = _ffi.DeviceBuffer.from_host(M)
    try:
        det, d_z = aS.diarize_clusters_device(d_m, M.shape[0], M.shape[1], 0, init_centers=init_of(g))
        Z = d_z.to_host(np.float64, M.size).reshape(M.shape).T
        d_z.free()
    finally:
        d_m.free()
    assert_close(det["mean"], g["mean"], "mean")
    assert_close(det["scale"], g["scale"], "scale")
    assert_close(Z[::7], g["z_sample"], "Z")
    assert_close(det["dim_colsum"], g["colsum"], "dimension distance sums")
    assert float(g["kept_margin"]) >= DIST_FLOOR
    assert np.array_equal(det["kept_dims"], g["kept_dims"])
    excluded = 0
    for k in (int(k) for k in g["ks"]):
        pre = "k%d_" % k
        if float(g[pre + "km_margin"]) < DIST_FLOOR or float(g[pre + "b_margin"]) < DIST_FLOOR:
            excluded += 1
            continue
        assert np.array_equal(det["labels"][k], g[pre + "labels"]), k
        assert det["n_iter"][k] == int(g[pre + "n_iter"]), k
        assert_close(det["centers"][k], g[pre + "centers"], "centres k=%d" % k)
        assert_close(det["inertia"][k], g[pre + "inertia"], "inertia k=%d" % k)
        assert_close(det["pair_sums"][k], g[pre + "pair_sums"], "pair sums k=%d" % k)
        assert_close(det["sil_a"][k], g[pre + "a"], "a k=%d" % k)
        assert_close(det["sil_b"][k], g[pre + "b"], "b k=%d" % k)
        assert_close(det["sil"][k], g[pre + "sil"], "sil k=%d" % k)
    if name in REAL:
        assert excluded == 0
    assert excluded < len(g["ks"])
    if excluded == 0:
        assert_close(det["scores"], g["scores"], "scores")
        assert float(g["imax_margin"]) >= DIST_FLOOR
        assert det["imax"] == int(g["imax"])


def hmm_cases():
    out = []
    for p in GOLDENS:
        g = load_golden(p)
        out += [(p, int(k)) for k in g["hmm_ks"]]
    return out


@pytest.mark.parametrize("path,k", hmm_cases(), ids=lambda v: golden_id(v) if isinstance(v, str) else str(v))
def test_diarize_features_matches_golden(gpu_lib, path, k):
    """The whole of steps 3-8: k = 9 is the sweep (the HMM is trained on the labels of the last k), other k are n_speakers."""
    g = load_golden(path)
    pre = "k%d_" % k
    assert float(g[pre + "hmm_margin"]) >= HMM_FLOOR and float(g[pre + "km_margin"]) >= DIST_FLOOR
    n_speakers = 0 if k == 9 else k
    cls, det = aS.diarize_features(g["M"], n_speakers, init_centers=init_of(g), return_details=True)
    assert np.array_equal(det["labels"][k], g[pre + "labels"])
    assert np.array_equal(det["hmm_states"], g[pre + "hmm_states"])
    assert cls.dtype == np.float64 and np.array_equal(cls, g[pre + "cls"])
    if "flags_gt" in g:
        got = aS.evaluate_speaker_diarization(cls, g["flags_gt"])
        print("purities", got, g[pre + "purity"])
        assert got[0] == g[pre + "purity"][0] and got[1] == g[pre + "purity"][1]
    if k == 9:
        assert det["ks"] == list(range(2, 10)) and det["imax"] == int(g["imax"])


def test_two_runs_are_bit_identical(gpu_lib):
    g = load_golden([p for p in GOLDENS if golden_id(p) == "diar_example"][0])
    runs = [aS.diarize_features(g["M"], 0, random_state=11, return_details=True) for _ in range(2)]
    (c0, d0), (c1, d1) = runs
    assert np.array_equal(c0, c1)
    for k in d0["ks"]:
        for key in ("labels", "centers", "sil_a", "sil_b", "sil", "pair_sums"):
            assert d0[key][k].tobytes() == d1[key][k].tobytes(), (key, k)
        assert d0["inertia"][k] == d1["inertia"][k] and d0["n_iter"][k] == d1["n_iter"][k]


def test_results_survive_shutdown_and_reinit(gpu_lib):
    """paa_shutdown frees and resets every global scratch buffer -- the HMM statistics' and the diarization work space
    register themselves like the others -- so the same calls after paa_init(0) allocate afresh and give the same bits."""
    g = load_golden([p for p in GOLDENS if golden_id(p) == "diar_example"][0])
    labels = (np.arange(g["M"].shape[1]) // 7) % 3

    def run():
        stats = aS.train_hmm_compute_statistics(g["M"], labels)
        return stats, aS.diarize_features(g["M"], 0, random_state=11, return_details=True)

    stats0, (c0, d0) = run()
    gpu_lib.paa_shutdown()
    _ffi.init(0)
    stats1, (c1, d1) = run()
    for a, b in zip(stats0, stats1):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.array_equal(c0, c1) and d0["ks"] == d1["ks"]
    for k in d0["ks"]:
        for key in ("labels", "centers", "sil", "pair_sums"):
            assert d0[key][k].tobytes() == d1[key][k].tobytes(), (key, k)


def test_constant_row_is_refused_by_the_hmm(gpu_lib):
    g = load_golden([p for p in GOLDENS if golden_id(p) == "diar_const"][0])
    with pytest.raises(ValueError):
        aS.diarize_features(g["M"], 0, init_centers=init_of(g))


def test_repeated_windows_pair_sums(gpu_lib):
    """The synthetic golden holds 24 identical windows: their mutual distances are exactly 0 in the difference form."""
    g = load_golden([p for p in GOLDENS if golden_id(p) == "diar_synth"][0])
    M = g["M"]
    n = M.shape[1]
    block = np.arange(n // 2 - 12, n // 2 + 12)
    assert np.all(M[:, block] == M[:, block[:1]])
    labels = np.zeros((1, n), dtype=np.int32)
    labels[0, block] = 1
    S = device_pair_sums(np.ascontiguousarray(M), labels, [2])
    assert S[0][1, 1] == 0.0
    assert_close(S[0], diar_ref.pair_sums(M.T, labels[0], 2), "pair sums")


def device_pair_sums(X, labels, ks):
    """paa_diar_dev_pair_sums_f64 on X [D][N] and labels [nk][N]."""
    lib = _ffi.lib()
    d_x, d_l = _ffi.DeviceBuffer.from_host(X), _ffi.DeviceBuffer.from_host(np.ascontiguousarray(labels, dtype=np.int32))
    ks_arr = np.array(ks, dtype=np.int32)
    out = np.empty((len(ks), 32, 32))
    try:
        _ffi.check(lib.paa_diar_dev_pair_sums_f64(d_x.ptr, X.shape[0], X.shape[1], X.shape[1], d_l.ptr,
                                                  ks_arr.ctypes.data_as(_ffi.c_i32p), len(ks), _ffi.as_f64p(out)))
    finally:
        d_x.free()
        d_l.free()
    return [out[i, :k, :k] for i, k in enumerate(ks)]


def device_kmeans(X, ks, inits, max_iter=300, tol=1e-4):
    """paa_diar_dev_kmeans_f64 on X [D][N]: per k (labels, centres, n_iter, inertia)."""
    lib = _ffi.lib()
    D, n = X.shape
    centers = np.zeros((len(ks), 32, D))
    for i, k in enumerate(ks):
        centers[i, :k] = inits[i]
    ks_arr = np.array(ks, dtype=np.int32)
    n_iter, inertia = np.zeros(len(ks), dtype=np.int32), np.empty(len(ks))
    d_x, d_l = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(X)), _ffi.DeviceBuffer(len(ks) * n * 4)
    try:
        _ffi.check(lib.paa_diar_dev_kmeans_f64(d_x.ptr, D, n, n, ks_arr.ctypes.data_as(_ffi.c_i32p), len(ks), _ffi.as_f64p(centers),
                                               tol * float(np.mean(np.var(X, axis=1))), max_iter, d_l.ptr,
                                               n_iter.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(inertia)))
        labels = d_l.to_host(np.int32, len(ks) * n).reshape(len(ks), n)
    finally:
        d_x.free()
        d_l.free()
    return [(labels[i].astype(np.int64), centers[i, :k].copy(), int(n_iter[i]), float(inertia[i])) for i, k in enumerate(ks)]


def planted(seed, n, d, k, spread=4.0):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((k, d)) * spread
    path = rng.integers(k, size=n)
    return (means[path] + rng.standard_normal((n, d))).T.copy(), path


@pytest.mark.parametrize("n,d,k", [(5, 3, 5), (6, 3, 5), (300, 1, 3), (500, 256, 4), (700, 20, 32), (33, 7, 32)])
def test_kmeans_edges(gpu_lib, n, d, k):
    """N = k, N = k + 1, D = 1, D = 256, k = 32 against the restatement, from its own seeding's centres."""
    X, _ = planted(100 + n, n, d, min(k, 6))
    init = X.T[diar_ref.seed_indices(X.T, k, 3)]
    ref = diar_ref.kmeans(X.T, k, init)
    assert ref["margin"] >= DIST_FLOOR
    labels, centers, n_iter, inertia = device_kmeans(X, [k], [init])[0]
    assert np.array_equal(labels, ref["labels"]) and n_iter == ref["n_iter"]
    assert_close(centers, ref["centers"], "centres")
    assert_close(inertia, ref["inertia"], "inertia")
    S = device_pair_sums(X, labels[None, :], [k])[0]
    assert_close(S, diar_ref.pair_sums(X.T, labels, k), "pair sums")


def test_kmeans_empty_cluster_is_relocated(gpu_lib):
    X, _ = planted(7, 200, 5, 3)
    init = np.vstack([X.T[:3], X.T.max(axis=0)[None, :] + 50.0])        # the fourth centre attracts no window
    ref = diar_ref.kmeans(X.T, 4, init)
    assert ref["margin"] >= DIST_FLOOR and len(np.unique(ref["labels"])) == 4
    labels, centers, n_iter, inertia = device_kmeans(X, [4], [init])[0]
    assert np.array_equal(labels, ref["labels"]) and n_iter == ref["n_iter"]
    assert_close(centers, ref["centers"], "centres")
    assert_close(inertia, ref["inertia"], "inertia")


def test_larger_seeded_case_matches_restatement(gpu_lib):
    """N = 3001 (not tile-aligned), seeded on the device with the restatement's draws."""
    X, _ = planted(42, 3001, 60, 5, spread=2.0)
    X[3] = X[3] * 0.0 + 1.5                                             # a constant row: scale 1, standardised to 0
    ref = diar_ref.cluster(X, 0, random_state=5)
    d_m = _ffi.DeviceBuffer.from_host(X)
    try:
        det, d_z = aS.diarize_clusters_device(d_m, X.shape[0], X.shape[1], 0, random_state=5)
        d_z.free()
    finally:
        d_m.free()
    assert ref["kept_margin"] >= DIST_FLOOR and np.array_equal(det["kept_dims"], ref["kept_dims"])
    assert_close(det["scale"], ref["scale"], "scale")
    checked = 0
    for k in ref["ks"]:
        r = ref["per_k"][k]
        if r["margin"] < DIST_FLOOR or r["b_margin"] < DIST_FLOOR:
            continue
        checked += 1
        assert np.array_equal(det["labels"][k], r["labels"]) and det["n_iter"][k] == r["n_iter"], k
        assert_close(det["centers"][k], r["centers"], "centres k=%d" % k)
        assert_close(det["inertia"][k], r["inertia"], "inertia k=%d" % k)
        assert_close(det["sil_a"][k], r["a"], "a k=%d" % k)
        assert_close(det["sil_b"][k], r["b"], "b k=%d" % k)
        assert_close(det["sil"][k], r["sil"], "sil k=%d" % k)
    assert checked >= 6


def synthetic_models():
    """Seeded SVMs of the shipped shapes (10 speakers, male / female) as load_model tuples."""
    out = []
    for n_classes, seed in ((10, 1), (2, 2)):
        m = svc_libsvm.synthetic_model([4] * n_classes, 136, seed)
        clf = audioTrainTest.SvcArrays(m["support_vectors"], m["n_support"], m["dual_coef"], -m["rho"], m["prob_a"], m["prob_b"],
                                       m["gamma"], "rbf", np.arange(n_classes, dtype=np.float64))
        rng = np.random.default_rng(seed)
        out.append((clf, rng.standard_normal(136) * 0.1, 0.5 + rng.random(136), ["c%d" % i for i in range(n_classes)], 1.0, 0.1,
                    0.05, 0.05, False))
    return out


def test_speaker_diarization_signal_end_to_end(gpu_lib):
    """The resident pipeline against the same pipeline assembled from the pieces that have their own tests."""
    from synth import synth_clip
    from pyaudioanalysis_amd import MidTermFeatures
    fs = 16000
    x = np.concatenate([synth_clip(s, 2 * fs) for s in (1, 2, 3, 1, 2, 3, 1)])
    models = synthetic_models()
    mid, _, _ = MidTermFeatures.mid_feature_extraction(x, fs, 1.0 * fs, 0.1 * fs, round(fs * 0.05), round(fs * 0.05))
    blocks = [mid]
    for clf, mean, std, *_ in models:
        _, proba = audioTrainTest.svc_model(clf).predict(mid, mean, std)
        blocks.append(proba.T + 1e-4)
    M = np.vstack(blocks)
    assert M.shape[0] == 148
    want, wd = aS.diarize_features(M, 3, random_state=4, return_details=True)
    got, gd = aS.speaker_diarization_signal(x, fs, 3, models=models, random_state=4, return_details=True)
    assert np.array_equal(gd["kept_dims"], wd["kept_dims"])
    assert np.array_equal(gd["labels"][3], wd["labels"][3]) and np.array_equal(got, want)
    stereo = np.stack([x, x], axis=1)
    assert np.array_equal(aS.speaker_diarization_signal(stereo, fs, 3, models=models, random_state=4), got)


def test_argument_errors(gpu_lib, tmp_path, monkeypatch):
    x = np.zeros(16000, dtype=np.int16)
    with pytest.raises(NotImplementedError, match="LDA"):
        aS.speaker_diarization_signal(x, 16000, 2, lda_dim=5, models=synthetic_models())
    with pytest.raises(NotImplementedError, match="LDA"):
        aS.speaker_diarization("nothing.wav", 2, lda_dim=5)
    monkeypatch.delenv(aS.DIAR_MODELS_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match=aS.DIAR_MODELS_ENV):
        aS.speaker_diarization_signal(x, 16000, 2)
    monkeypatch.setenv(aS.DIAR_MODELS_ENV, str(tmp_path))
    with pytest.raises(FileNotFoundError, match="svm_rbf_speaker_10"):
        aS.speaker_diarization_signal(x, 16000, 2)
    M = np.random.default_rng(0).standard_normal((6, 3))
    with pytest.raises(ValueError):
        aS.diarize_features(M, 4)                      # N < k
    with pytest.raises(ValueError):
        aS.diarize_features(np.empty((6, 0)), 2)       # N < 1
    with pytest.raises(ValueError):
        aS.diarize_features(np.zeros((6, 40)), 33)     # k > 32
    with pytest.raises(ValueError):
        aS.diarize_features(np.zeros((257, 40)), 2)    # D > 256
