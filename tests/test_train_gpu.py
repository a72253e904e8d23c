"""GPU tests of classifier tuning and training: the kNN split-sweep kernel (knn_split_kernel of kernels_knn.hpp through
paa_knn_splits_f64 / audioTrainTest.knn_split_predict), evaluate_classifier for the six classifier types and
extract_features_and_train, against the train_* goldens of the unmodified reference (scripts/make_train_golden.py) and the
NumPy restatements (tests/knn_ref.py, tests/train_ref.py)."""
import contextlib
import io
import os

import numpy as np
import pytest

import knn_ref
import train_ref
from pyaudioanalysis_amd import audioTrainTest

pytestmark = pytest.mark.gpu

QPB, TILE, STEP, K_INSTANCES = 16, 16, 8, (1, 2, 4, 8, 16, 32)          # checked against the library in test_geometry


def test_geometry(gpu_lib):
    """The edge grids below aim at these numbers."""
    assert audioTrainTest.knn_split_geometry() == (QPB, TILE, STEP, K_INSTANCES)


def _neighbours_agree(nb, want, D):
    """Equal neighbour lists up to the order of neighbours whose squared distances agree to 1e-12 relative (the kernel and
    NumPy sum the squares in different orders): the rule of test_knn_gpu.py."""
    for v in range(nb.shape[0]):
        if np.array_equal(nb[v], want[v]):
            continue
        assert sorted(nb[v].tolist()) == sorted(want[v].tolist()), v
        d = D[v, nb[v]]
        assert np.all(np.abs(d - D[v, want[v]]) <= 1e-12 * np.maximum(d, 1e-300)), v


def _check_jobs(X, labels, jobs, exact, skip=()):
    """One launch for all jobs; every job against knn_ref.classify on its standardised split, and the padding of the raw
    outputs.  Returns the result."""
    res = audioTrainTest.knn_split_predict(X, labels, jobs, proba=True, neighbors=True)
    k_launch = min(K for K in K_INSTANCES if K >= max(j[4] for j in jobs))
    assert res.neighbors.shape == (res.test_off[-1], k_launch) and res.label.shape == (res.test_off[-1],)
    assert res.proba.shape[1] == max(res.n_classes)
    for j, (tr, te, mean, scale, k) in enumerate(jobs):
        lab, P, nb = res.job(j)
        assert lab.shape == (len(te),)
        if len(te) == 0 or j in skip:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            T, Q = (X[tr] - mean) / scale, (X[te] - mean) / scale
        want_lab, want_P, want_nb = knn_ref.classify(T, np.asarray(labels)[tr], k, Q)
        assert res.n_classes[j] == want_P.shape[1], j
        assert np.array_equal(lab, want_lab), j
        assert np.array_equal(P, want_P), j
        if exact:
            assert np.array_equal(nb, want_nb), j
        else:
            _neighbours_agree(nb, want_nb, knn_ref.squared_distances(T, Q))
        a, b = int(res.test_off[j]), int(res.test_off[j + 1])
        assert not res.proba[a:b, res.n_classes[j]:].any() and np.all(res.neighbors[a:b, k:] == -1), j
    return res


@pytest.mark.parametrize("name", ["train_knn_three", "train_knn_rare"])
def test_golden_jobs_match_reference_and_restatement(gpu_lib, name):
    """Every job of every run of a golden in ONE call: the labels are the unmodified reference's per-split predictions, with
    no vector set aside; P and the neighbours are the restatement's."""
    g = train_ref.load_golden(name)
    X, y = train_ref.features_to_matrix(train_ref.golden_features(g))
    jobs, want = [], []
    for r in train_ref.golden_runs(g):
        jobs += train_ref.run_jobs(g, r)
        want.append(g[r + "pred"])
    res = _check_jobs(X, y, jobs, exact=False)
    assert np.array_equal(res.label, np.concatenate(want))
    assert len({int(n) for n in res.n_classes}) > 1 or name == "train_knn_three"     # the rare case has splits without a class
    # without the optional outputs: the same labels
    assert np.array_equal(audioTrainTest.knn_split_predict(X, y, jobs).label, res.label)


def _int_samples(rng, n_samples, n_dims, n_labels):
    X = rng.integers(-1, 2, (n_samples, n_dims)).astype(np.float64)
    labels = (np.arange(n_samples) % n_labels).astype(np.float64)
    return X, labels


def _int_job(rng, n_samples, n_train, n_test, k, n_dims, scale=1.0):
    """Permuted lists; the test list overlaps the train list of this and of other jobs."""
    tr = rng.permutation(n_samples)[:n_train] if n_train <= n_samples else rng.integers(0, n_samples, n_train)
    te = rng.permutation(n_samples)[:n_test] if n_test <= n_samples else rng.integers(0, n_samples, n_test)
    return tr, te, np.zeros(n_dims), np.full(n_dims, scale), k


TEST_LENGTHS = (0, 1, 15, 16, 17, 33)
TRAIN_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 33)
INT_K = (1, 2, 8, 9, 31, 32)


def test_integer_grid_list_lengths_and_k(gpu_lib):
    """Integer coordinates: every d^2 is exact, so labels, P and neighbours compare exactly.  Test lists around the 16
    queries of a workgroup, train lists around the 8 rows of a step and the 16 of a tile, k at the ends of every K instance,
    k = 1 and k = 32 in ONE call (launched at K = 32), k above the train-list length."""
    rng = np.random.default_rng(1)
    X, labels = _int_samples(rng, 40, 9, 3)
    jobs = [_int_job(rng, 40, n_train, TEST_LENGTHS[(i + j) % 6], INT_K[(i + 2 * j) % 6], 9)
            for i, n_train in enumerate(TRAIN_LENGTHS) for j in range(3)]
    assert {len(j[1]) for j in jobs} == set(TEST_LENGTHS) and {j[4] for j in jobs} == set(INT_K)
    assert any(j[4] > len(j[0]) for j in jobs)
    _check_jobs(X, labels, jobs, exact=True)
    # a sweep at a smaller K instance, and one job alone
    for k_set in ((1,), (1, 2), (3, 4), (8, 5), (9, 16)):
        _check_jobs(X, labels, [_int_job(rng, 40, 33, 17, k, 9) for k in k_set], exact=True)
    # scale 2: the division is exact (halves), d^2 a multiple of 0.25
    _check_jobs(X, labels, [_int_job(rng, 40, 17, 33, 9, 9, scale=2.0), _int_job(rng, 40, 33, 16, 32, 9)], exact=True)


@pytest.mark.parametrize("n_dims", [1, 7, 8, 9, 255, 256])
def test_integer_grid_dims(gpu_lib, n_dims):
    rng = np.random.default_rng(100 + n_dims)
    X, labels = _int_samples(rng, 40, n_dims, 4)
    _check_jobs(X, labels, [_int_job(rng, 40, 33, 17, 9, n_dims), _int_job(rng, 40, 16, 16, 2, n_dims),
                            _int_job(rng, 40, 9, 1, 32, n_dims, scale=2.0)], exact=True)


def test_integer_grid_classes_and_missing_classes(gpu_lib):
    """1, 2, 63 and 64 classes; a train list that lacks the highest class (n_classes shrinks, nothing else changes), one that
    lacks a middle class (n_classes shrinks and the rows of the highest class vote for no class), labels of -1."""
    rng = np.random.default_rng(2)
    X, labels = _int_samples(rng, 200, 8, 64)
    by_class = [np.flatnonzero(labels == c) for c in range(64)]
    everything = rng.permutation(200)
    no_highest = rng.permutation(np.concatenate(by_class[:63]))
    no_middle = rng.permutation(np.concatenate(by_class[:30] + by_class[31:]))
    two = rng.permutation(np.concatenate(by_class[:2]))
    te = rng.permutation(200)[:33]
    ones, zeros = np.ones(8), np.zeros(8)
    jobs = [(everything, te, zeros, ones, 9), (no_highest, te, zeros, ones, 9), (no_middle, te, zeros, ones, 32),
            (by_class[0], te[:17], zeros, ones, 2), (two, te[:16], zeros, ones, 3), (no_middle[:40], te[:15], zeros, ones, 1)]
    res = _check_jobs(X, labels, jobs, exact=True)
    assert res.n_classes.tolist()[:5] == [64, 63, 63, 1, 2]
    # the rows of class 63 are among the neighbours of the job without a middle class, and their votes are missing from P
    lab, P, nb = res.job(2)
    voted_63 = np.array([np.count_nonzero(labels[no_middle[row]] == 63) for row in nb])
    assert voted_63.any() and np.allclose(P.sum(axis=1), (32 - voted_63) / 32.0)
    with_minus = (np.arange(200) % 5).astype(np.float64)
    with_minus[rng.permutation(200)[:60]] = -1          # -1 is a label value of its own when the classes are counted: 6, the last empty
    res = _check_jobs(X, with_minus, jobs[:3], exact=True)
    assert res.n_classes.tolist() == [6, 6, 6] and not res.proba[:, 5].any() and np.all(res.proba.sum(axis=1) < 1.0 + 1e-12)


def test_ties_break_by_train_list_position(gpu_lib):
    """Duplicated sample rows listed in DESCENDING sample index: among equal distances the first in the train list wins, not
    the lowest sample index."""
    rng = np.random.default_rng(3)
    X, _ = _int_samples(rng, 24, 5, 2)
    X[12:] = X[:12]                                     # sample i + 12 duplicates sample i
    labels = np.concatenate([np.zeros(12), np.ones(12)])    # ... under the other label
    tr = np.arange(23, -1, -1)                          # the copy (label 1) comes first in the list
    te = np.arange(12)
    res = _check_jobs(X, labels, [(tr, te, np.zeros(5), np.ones(5), 1), (tr[::-1].copy(), te, np.zeros(5), np.ones(5), 1),
                                  (tr, te, np.zeros(5), np.ones(5), 2)], exact=True)
    assert np.all(res.job(0)[0] == 1) and np.all(res.job(1)[0] == 0)
    first = res.job(0)[2][:, 0]
    assert np.all(tr[first] >= 12)                      # the neighbour is the copy: list position, not sample index


def test_zero_scale_gives_no_neighbours_in_that_job_only(gpu_lib):
    """scale = 0 where the queries equal the mean: 0 / 0 = NaN queries, which get label 0, P = 0 and no neighbours; the
    other jobs of the call are unaffected."""
    rng = np.random.default_rng(4)
    X, labels = _int_samples(rng, 40, 9, 3)
    good = [_int_job(rng, 40, 17, 17, 2, 9), _int_job(rng, 40, 33, 16, 9, 9)]
    tr, te = rng.permutation(40)[:20], rng.permutation(40)[:18]
    X[te, 4] = 0.0
    scale = np.ones(9)
    scale[4] = 0.0
    jobs = [good[0], (tr, te, np.zeros(9), scale, 3), good[1]]
    res = _check_jobs(X, labels, jobs, exact=True, skip=(1,))
    lab, P, nb = res.job(1)
    assert not lab.any() and not P.any() and np.all(nb == -1)


def test_random_jobs_match_restatement(gpu_lib):
    """Gaussian samples, permuted overlapping lists, several workgroups and tiles per job, the k of every job drawn."""
    X, labels, jobs = train_ref.seeded_jobs(150, 37, 7, seed=8)
    _check_jobs(X, labels, jobs, exact=False)


def test_same_answers_through_the_model_path(gpu_lib):
    """Three jobs of a golden as uploaded models (the training rows standardised on the host, knn_kernel): labels and P bit
    for bit."""
    g = train_ref.load_golden("train_knn_three")
    X, y = train_ref.features_to_matrix(train_ref.golden_features(g))
    jobs = [train_ref.run_jobs(g, "r0_")[s] for s in (0, 13, 31)]
    res = audioTrainTest.knn_split_predict(X, y, jobs, proba=True)
    for j, (tr, te, mean, scale, k) in enumerate(jobs):
        model = audioTrainTest.Knn((X[tr] - mean) / scale, y[tr], k)
        lab, P = audioTrainTest.knn_predict(model, np.ascontiguousarray(X[te].T), mean, scale)
        assert np.array_equal(lab, res.job(j)[0]) and np.array_equal(P, res.job(j)[1])


def _run(fn, *args, **kw):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = fn(*args, **kw)
    return ret, out.getvalue()


@pytest.mark.parametrize("name,r", [("train_knn_three", "r0_"), ("train_knn_three", "r1_"), ("train_knn_rare", "r0_"),
                                    ("train_knn_rare", "r1_"), ("train_knn_rare", "r2_"), ("train_knn_rare", "r3_")])
def test_evaluate_classifier_knn_equals_the_reference(gpu_lib, name, r):
    pytest.importorskip("sklearn")
    g = train_ref.load_golden(name)
    names = [str(s) for s in g["class_names"]]
    np.random.seed(int(g[r + "seed"]))
    (ret, cms, preds), text = _run(audioTrainTest.evaluate_classifier_full, train_ref.golden_features(g), names, "knn", g["params"],
                                   int(g[r + "mode"]), train_ref.run_ids(g, r), n_exp=int(g[r + "n_exp"]),
                                   train_percentage=float(g[r + "train_percentage"]))
    assert ret == g[r + "ret"] and type(ret) is type(g["params"][0])
    assert np.array_equal(np.array(cms), g[r + "cms"])
    assert np.array_equal(np.concatenate([p for row in preds for p in row]), g[r + "pred"])
    assert text == str(g[r + "text"])
    assert np.array_equal(np.random.get_state()[1], g[r + "rng_after"])
    np.random.seed(int(g[r + "seed"]))
    ret2, text2 = _run(audioTrainTest.evaluate_classifier, train_ref.golden_features(g), names, "knn", g["params"], int(g[r + "mode"]),
                       train_ref.run_ids(g, r), int(g[r + "n_exp"]), float(g[r + "train_percentage"]))
    assert ret2 == ret and text2 == text


@pytest.mark.parametrize("r", ["r%d_" % i for i in range(5)])
def test_evaluate_classifier_sklearn_types_equal_the_restatement(gpu_lib, r):
    """The five scikit-learn types on the golden's data: the restatement (scikit-learn's per-vector predict) and
    evaluate_classifier (the device models) under the same seed in this process."""
    pytest.importorskip("sklearn")
    g = train_ref.load_golden("train_sklearn_small")
    feats, names = train_ref.golden_features(g), [str(s) for s in g["class_names"]]
    kind, params, n_exp, pct = str(g[r + "kind_name"]), g[r + "params"], int(g[r + "n_exp"]), float(g[r + "train_percentage"])
    np.random.seed(int(g[r + "seed"]))
    want_ret, want_cms, want_preds, want_text = train_ref.evaluate(
        feats, names, params, 1, n_exp, train_ref.random_split_source(sum(len(f) for f in feats), pct), train_ref.sklearn_fit(kind),
        train_ref.sklearn_classify)
    np.random.seed(int(g[r + "seed"]))
    (ret, cms, preds), text = _run(audioTrainTest.evaluate_classifier_full, feats, names, kind, params, 1, None, n_exp=n_exp,
                                   train_percentage=pct)
    assert ret == want_ret
    assert np.array_equal(np.array(cms), want_cms)
    assert np.array_equal(np.concatenate([p for row in preds for p in row]), np.concatenate(want_preds))
    assert text == want_text


def _write_dir(g, root):
    import scipy.io.wavfile as wavfile
    for name in g["file_names"]:
        name = str(name)
        os.makedirs(os.path.join(root, os.path.dirname(name)), exist_ok=True)
        wavfile.write(os.path.join(root, name), int(g["fs"]), g["wav_x_" + name])
    return [os.path.join(root, "tones"), os.path.join(root, "bursts")]


def test_extract_features_and_train_knn(gpu_lib, tmp_path):
    """The reference's extract_features_and_train for "knn" on the golden's two class folders: the eleven saved values."""
    pytest.importorskip("sklearn")
    import pickle
    g = train_ref.load_golden("train_dir_small")
    paths = _write_dir(g, str(tmp_path))
    model = str(tmp_path / "model_knn")
    np.random.seed(int(g["seed"]))
    _, text = _run(audioTrainTest.extract_features_and_train, paths, float(g["mid_window"]), float(g["mid_step"]),
                   float(g["short_window"]), float(g["short_step"]), "knn", model)
    assert str(g["selected_line"]) in text.splitlines()
    with open(model, "rb") as fo:
        saved = [pickle.load(fo) for _ in range(11)]
    features, labels, mean, std, class_names, neighbors, mid_window, mid_step, short_window, short_step, compute_beat = saved
    assert neighbors == g["saved_neighbors"] and class_names == [str(s) for s in g["saved_class_names"]]
    assert (mid_window, mid_step, short_window, short_step, compute_beat) == \
        (float(g["saved_mid_window"]), float(g["saved_mid_step"]), float(g["saved_short_window"]), float(g["saved_short_step"]),
         bool(g["saved_compute_beat"]))
    assert np.array_equal(np.array(labels), g["saved_labels"])
    for got, key in ((features, "saved_features"), (mean, "saved_mean"), (std, "saved_std")):
        got, ref = np.array(got), g[key]
        err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print("%s: max relative deviation %.3g, max absolute %.3g" % (key, err.max(), np.abs(got - ref).max()))
    for got, key in ((features, "saved_features"), (mean, "saved_mean"), (std, "saved_std")):
        assert np.allclose(np.array(got), g[key], rtol=1e-9, atol=1e-12), key
    loaded = audioTrainTest.load_model_knn(model)
    assert len(loaded) == 9 and loaded[0].neighbors == neighbors and loaded[3] == class_names
    for wav, want in (("tones/t03.wav", "tones"), ("bursts/b07.wav", "bursts")):
        class_id, P, names = audioTrainTest.file_classification(os.path.join(str(tmp_path), wav), model, "knn")
        assert names[int(class_id)] == want and P.shape == (2,)


def test_extract_features_and_train_svm(gpu_lib, tmp_path):
    pytest.importorskip("sklearn")
    g = train_ref.load_golden("train_dir_small")
    paths = _write_dir(g, str(tmp_path))
    model = str(tmp_path / "model_svm")
    np.random.seed(int(g["seed"]))
    _run(audioTrainTest.extract_features_and_train, paths, float(g["mid_window"]), float(g["mid_step"]), float(g["short_window"]),
         float(g["short_step"]), "svm", model)
    assert os.path.isfile(model) and os.path.isfile(model + "MEANS")
    loaded = audioTrainTest.load_model(model)
    assert len(loaded) == 9 and loaded[3] == ["tones", "bursts"] and loaded[1].shape == (136,)
    class_id, P, names = audioTrainTest.file_classification(os.path.join(str(tmp_path), "tones/t03.wav"), model, "svm")
    assert names == ["tones", "bursts"] and P.shape == (2,) and class_id in (0.0, 1.0)


def test_one_job_list_through_both_sweeps(gpu_lib):
    """The same (train_idx, test_idx, mean, scale) jobs through knn_split_predict and svm_split_fit_predict: 3 classes x 12 rows x
    5 dims of small integers; an empty test list, 17 test rows (one past the 16 queries of a kNN workgroup), 33 (one past the 32
    rows of an SVM vote workgroup) and a training list without class 2.  Both results carve the test rows up alike, and each
    job's slice equals, bit for bit, what the same function returns for that job alone."""
    rng = np.random.default_rng(77)
    y = np.repeat(np.arange(3), 12)
    X = (rng.integers(-3, 4, (36, 5)) + 2 * y[:, None]).astype(np.float64)
    perm = rng.permutation(36)
    lists = [(perm[:30], perm[:0]), (perm[5:], perm[:17]), (perm, perm[:33]), (np.flatnonzero(y < 2)[::-1], perm[20:])]
    stats = [(np.zeros(5), np.ones(5)), (np.arange(5.0), np.full(5, 2.0)), (np.ones(5), np.full(5, 0.5)), (-np.ones(5), np.ones(5))]
    ks, Cs = (1, 3, 32, 4), (0.5, 1.0, 20.0, 1.0)
    n_test = [0, 17, 33, 16]
    knn_jobs = [l + s + (k,) for l, s, k in zip(lists, stats, ks)]
    svm_jobs = [l + s + (C,) for l, s, C in zip(lists, stats, Cs)]
    knn = audioTrainTest.knn_split_predict(X, y, knn_jobs, proba=True, neighbors=True)
    svm = audioTrainTest.svm_split_fit_predict(X, y, svm_jobs, decision=True)
    want_off = np.concatenate([[0], np.cumsum(n_test)])
    assert np.array_equal(knn.test_off, want_off) and np.array_equal(svm.test_off, want_off)
    assert knn.test_off.dtype == svm.test_off.dtype == np.int64
    assert knn.n_classes.tolist() == [3, 3, 3, 2] and [c.tolist() for c in svm.classes] == [[0, 1, 2]] * 3 + [[0, 1]]
    assert svm.task_off.tolist() == [0, 3, 6, 9, 10] and svm.decision.shape == (66, 3) and knn.proba.shape == (66, 3)
    for j in range(4):
        k_got, s_got = knn.job(j), svm.job(j)
        assert k_got[0].shape == s_got[0].shape == (n_test[j],)
        assert k_got[1].shape == (n_test[j], knn.n_classes[j]) and k_got[2].shape == (n_test[j], ks[j])
        assert s_got[1].shape == (n_test[j], len(svm.classes[j]) * (len(svm.classes[j]) - 1) // 2)
        k_alone = audioTrainTest.knn_split_predict(X, y, [knn_jobs[j]], proba=True, neighbors=True).job(0)
        s_alone = audioTrainTest.svm_split_fit_predict(X, y, [svm_jobs[j]], decision=True).job(0)
        for got, want in zip(k_got + s_got, k_alone + s_alone):
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), j
    assert np.all(svm.status == audioTrainTest.SMO_CONVERGED) and np.all(np.isin(svm.job(3)[0], [0, 1]))
