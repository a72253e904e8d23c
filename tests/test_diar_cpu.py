"""CPU checks of speaker diarization: the NumPy restatement tests/diar_ref.py against the SciPy / scikit-learn stage outputs
stored in the goldens (scripts/make_diar_golden.py), a forced empty cluster against scikit-learn's KMeans, the host-side
evaluate_speaker_diarization against the reference's stored results, the restated seeding, and the C ABI."""
import os
import re
import warnings

import numpy as np
import pytest

import diar_ref
from conftest import ROOT, golden_files, golden_id, load_golden
from pyaudioanalysis_amd import _ffi
from pyaudioanalysis_amd import audioSegmentation as aS

TIGHT = 1e-9
GOLDENS = golden_files("diar")
SYMBOLS = ["paa_diar_dev_standardize_f64", "paa_diar_dev_select_rows_f64", "paa_diar_dev_dim_distances_f64",
           "paa_diar_dev_sqdist_points_f64", "paa_diar_dev_get_points_f64", "paa_diar_dev_kmeans_f64", "paa_diar_dev_pair_sums_f64"]


def assert_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1.0)
    assert err <= TIGHT, (what, err)


def test_goldens_present_and_small():
    assert sorted(golden_id(p) for p in GOLDENS) == ["diar_const", "diar_example", "diar_example2", "diar_example_2s", "diar_synth"]
    for p in GOLDENS:
        assert os.path.getsize(p) < 1000000, p


@pytest.mark.parametrize("path", GOLDENS, ids=golden_id)
def test_restatement_matches_golden_stages(path):
    g = load_golden(path)
    init = {int(k): g["k%d_init" % k] for k in g["ks"]}
    r = diar_ref.cluster(g["M"], 0, init_centers=init)
    assert_close(r["mean"], g["mean"], "mean")
    assert_close(r["scale"], g["scale"], "scale")
    assert_close(r["Z"][::7], g["z_sample"], "Z")
    assert_close(r["colsum"], g["colsum"], "colsum")
    assert np.array_equal(r["kept_dims"], g["kept_dims"])
    assert r["kept_margin"] == float(g["kept_margin"]) >= 1e-6
    for k in (int(k) for k in g["ks"]):
        pre, got = "k%d_" % k, r["per_k"][k]
        assert np.array_equal(got["labels"], g[pre + "labels"]) and got["n_iter"] == int(g[pre + "n_iter"]), k
        assert_close(got["centers"], g[pre + "centers"], "centres")
        assert_close(got["inertia"], g[pre + "inertia"], "inertia")
        assert_close(got["a"], g[pre + "a"], "a")
        assert_close(got["b"], g[pre + "b"], "b")
        assert_close(got["sil"], g[pre + "sil"], "sil")
        # every (case, k) supports the exact comparisons of the GPU suite: nothing is excluded
        assert got["margin"] >= 1e-6 and got["b_margin"] >= 1e-6, (k, got["margin"], got["b_margin"])
    assert r["imax"] == int(g["imax"]) and r["imax_margin"] >= 1e-6
    for k in (int(k) for k in g["hmm_ks"]):
        pre = "k%d_" % k
        states, margins, cls = diar_ref.smooth(r["Z"], r["per_k"][k]["labels"])
        assert margins.min() >= 1e-3
        assert np.array_equal(states, g[pre + "hmm_states"]) and np.array_equal(cls, g[pre + "cls"])


def test_medfilt_matches_scipy():
    from scipy.signal import medfilt
    x = np.random.default_rng(1).integers(0, 5, 57).astype(np.float64)
    assert np.array_equal(diar_ref.medfilt5(x), medfilt(x, 5))
    assert np.array_equal(diar_ref.medfilt5(x[:3]), medfilt(x[:3], 5))


def test_forced_empty_cluster_against_sklearn():
    from sklearn.cluster import KMeans
    rng = np.random.default_rng(3)
    X = np.vstack([rng.standard_normal((60, 4)) + m for m in (0.0, 6.0, -6.0)])
    init = np.vstack([X[0], X[70], X[130], X.max(axis=0) + 40.0])      # the fourth centre attracts no point
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=4, init=init, n_init=1).fit(X)
    r = diar_ref.kmeans(X, 4, init)
    assert len(np.unique(km.labels_)) == 4
    assert np.array_equal(r["labels"], km.labels_) and r["n_iter"] == km.n_iter_
    assert_close(r["centers"], km.cluster_centers_, "centres")
    assert_close(r["inertia"], km.inertia_, "inertia")


@pytest.mark.parametrize("path", [p for p in GOLDENS if "flags_gt" in load_golden(p)], ids=golden_id)
def test_purities_match_the_reference(path):
    g = load_golden(path)
    for k in (int(k) for k in g["hmm_ks"]):
        want = g["k%d_purity" % k]
        for fn in (aS.evaluate_speaker_diarization, diar_ref.evaluate):
            got = fn(g["k%d_cls" % k], g["flags_gt"])
            assert got[0] == want[0] and got[1] == want[1], (k, got, want)


def test_recorded_good_run_of_the_example():
    g = load_golden([p for p in GOLDENS if golden_id(p) == "diar_example"][0])
    assert g["k4_purity"].min() >= 0.9          # the golden documents a good run; tests assert equality with it


def test_seeding_is_reproducible():
    Z = np.random.default_rng(2).standard_normal((300, 9))
    a, b = diar_ref.seed_indices(Z, 7, 5), diar_ref.seed_indices(Z, 7, 5)
    assert np.array_equal(a, b) and len(set(a.tolist())) == 7 and a.min() >= 0 and a.max() < 300
    assert not np.array_equal(a, diar_ref.seed_indices(Z, 7, 6))
    rs = np.random.RandomState(5)
    assert np.array_equal(diar_ref.seed_indices(Z, 7, rs), a)


def test_abi_symbols():
    text = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(paa_[a-z0-9_]+)\s*\(", text))
    lib = _ffi.lib()
    for s in SYMBOLS:
        assert s in declared and s in _ffi.EXPORTED_SYMBOLS and hasattr(lib, s), s


def test_host_side_errors(monkeypatch, tmp_path):
    with pytest.raises(NotImplementedError, match="LDA"):
        aS.speaker_diarization("nothing.wav", 2, lda_dim=5)
    monkeypatch.delenv(aS.DIAR_MODELS_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match=aS.DIAR_MODELS_ENV):
        aS.speaker_diarization("nothing.wav", 2)
    with pytest.raises(FileNotFoundError, match="svm_rbf_speaker_10"):
        aS.speaker_diarization("nothing.wav", 2, models_dir=str(tmp_path))
