"""CPU tests of the references and generators behind the model edge suites (tests/test_{knn,forest,hmm,diar}_edges_gpu.py):
every np.longdouble restatement against the FP64 one on benign input (and against SciPy where it imports), and every
designed input's promise -- the integer kNN cases really hold ties of each kind, the forest probes fall on both sides of
every boundary, the twin-state sequences tie on both sides of segment seams while every other decision clears the margin
floor, the k-means designs are exact.  Also the condition of the ambiguity cap of tests/test_knn_gpu.py."""
import numpy as np
import pytest

import diar_ref
import forest_ref
import hmm_ref
import knn_ref

DIST_FLOOR = 1e-6
MIN_MARGIN = 1e-3


# --------------------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("name", sorted(knn_ref.SHAPES) + sorted(knn_ref.EDGES))
def test_knn_seeded_cases_stay_within_the_ambiguity_cap(name):
    """What _check_against_restatement of test_knn_gpu.py may set aside, from knn_ref alone: no vector at all."""
    F, labels, k, feats, mean, std = knn_ref.shape_case(name) if name in knn_ref.SHAPES else knn_ref.edge_case(name)
    amb = knn_ref.ambiguous_vectors(F, labels, k, (feats.T - mean) / std)
    assert int(amb.sum()) <= knn_ref.AMBIGUOUS_CAP * amb.shape[0], (name, int(amb.sum()))


def test_knn_integer_cases_are_exact_and_tied():
    grid = knn_ref.integer_grid()
    assert len(grid) == 60 and {g[0] for g in grid} == set(knn_ref.INT_N_TRAIN) and {g[1] for g in grid} == set(knn_ref.INT_K)
    for j, vals in ((2, knn_ref.INT_DIMS), (3, knn_ref.INT_CLASSES), (4, knn_ref.INT_N_VEC)):
        assert {g[j] for g in grid} == set(vals)
    total = {"kth": 0, "lanes": 0, "tiles": 0, "votes": 0}
    for n_train, k, n_dims, n_classes, n_vec in grid:
        F, labels, X = knn_ref.integer_case(n_train, n_dims, n_classes, n_vec, 1000 * n_train + k)
        D = knn_ref.squared_distances(F, X)
        assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 40          # exact integers in any order of summation
        Dl = np.stack([np.sum((F.astype(np.longdouble) - x) ** 2, axis=1) for x in X])
        assert np.array_equal(D, Dl.astype(np.float64))
        lab, c = knn_ref.label_indices(labels)
        assert c == min(n_classes, n_train) and not np.any(lab[lab >= 0] % 2 == 1)     # the odd classes have no training row
        assert c < 2 or np.any(lab < 0)
        for key, v in knn_ref.tie_kinds(F, labels, k, X).items():
            total[key] += v
    assert min(total.values()) >= 20, total
    # the tie-rich case alone holds every kind, at every k it is run with
    for k in (1, 8, 32):
        F, labels, X = knn_ref.integer_case(33, 7, 8, 17, 5)
        kinds = knn_ref.tie_kinds(F, labels, k, X)
        assert kinds["kth"] >= (5 if k < 32 else 0) and kinds["lanes"] >= 5 and kinds["tiles"] >= (5 if k > 1 else 1), (k, kinds)
        assert kinds["votes"] >= (1 if k == 8 else 0), (k, kinds)


def test_knn_overflow_case():
    F, labels, k, X = knn_ref.overflow_case()
    D = knn_ref.squared_distances(F, X)
    assert np.isinf(D).any(axis=1).all() and (np.isfinite(D).sum(axis=1) < k).all() and not np.isnan(D).any()
    fin = D[np.isfinite(D)]
    assert np.array_equal(fin, np.round(fin))
    idx, P, nb = knn_ref.classify(F, labels, k, X)
    assert np.all(nb >= 0) and all(np.isfinite(D[v, nb[v, 0]]) and np.isinf(D[v, nb[v, -1]]) for v in range(X.shape[0]))


# ------------------------------------------------------------------------------------------------------------ forests
def test_forest_probes_fall_on_both_sides_of_every_boundary():
    B = forest_ref.boundaries()
    X, right = forest_ref.boundary_rows()
    for f, (name, thr, miss, probes) in enumerate(B):
        sides = [forest_ref.boundary_side(p, thr, miss) for p in probes]
        assert True in sides and False in sides, name
        assert right[:, f].any() and (~right[:, f]).any(), name
        assert forest_ref.boundary_side(forest_ref.BENIGN, thr, miss), name
    by = {b[0]: b for b in B}
    # the listed places: equal after the cast and one ulp to either side
    _, thr, _, p = by["equal_f32"]
    assert np.float32(p[0]) == np.float32(thr) and np.float32(p[1]) > np.float32(thr) > np.float32(p[2])
    assert np.nextafter(np.float32(thr), np.float32(np.inf)) == np.float32(p[1])
    # rounding across a threshold in float32 but not in FP64
    for name in ("rounds_down_across", "rounds_up_across"):
        _, thr, miss, p = by[name]
        assert (p[0] <= thr) != forest_ref.boundary_side(p[0], thr, miss), name
        assert (p[1] <= thr) == forest_ref.boundary_side(p[1], thr, miss), name
    _, thr, miss, p = by["zero"]
    assert np.signbit(p[0]) and forest_ref.boundary_side(p[0], thr, miss) and not forest_ref.boundary_side(p[2], thr, miss)
    assert p[4] > 0 and forest_ref.boundary_side(p[4], thr, miss) and not forest_ref.boundary_side(p[5], thr, miss)
    _, thr, miss, p = by["subnormal"]
    assert 0 < thr < float(np.finfo(np.float32).tiny)
    _, thr, miss, p = by["flt_max"]
    x32 = forest_ref.to_x32(np.array(p))
    assert p[1] > forest_ref.F32_MAX and x32[1] == np.float32(forest_ref.F32_MAX) and np.isposinf(x32[2]) and np.isneginf(x32[3])
    assert float(np.nextafter(p[2], 0.0)) == p[1]


@pytest.mark.parametrize("kind,n_classes,reverse", [("averaged", 3, False), ("averaged", 9, True), ("boosted", 2, False)])
def test_forest_boundary_model_scores_are_the_decision_mask(kind, n_classes, reverse):
    model, order = forest_ref.boundary_model(kind, n_classes, reverse)
    X, right = forest_ref.boundary_rows()
    labels, proba, raw = forest_ref.predict(model, X, check=False)
    assert np.array_equal(raw[:, -1], forest_ref.boundary_mask(right, order))
    X32 = forest_ref.to_x32(X)
    assert np.array_equal(labels == -1, np.isinf(X32).any(axis=1) & ~(np.isnan(X32).any(axis=1) & (kind == "boosted")))
    with pytest.raises(ValueError):
        forest_ref.predict(model, X)


def test_forest_links_in_longdouble():
    rng = np.random.default_rng(3)
    for K in (1, 3, 9):
        raw = rng.standard_normal((50, K)) * 5
        model = forest_ref.score_model(raw)
        labels, proba, got = forest_ref.predict(model, np.arange(50.0)[:, None])
        assert np.array_equal(got, raw)
        assert np.max(np.abs(proba - forest_ref.boosted_proba_ld(raw))) <= 1e-15
    sat = forest_ref.boosted_proba_ld(np.array([[1000.0], [-1000.0], [0.0]])).astype(np.float64)
    assert sat.tolist() == [[0.0, 1.0], [1.0, 0.0], [0.5, 0.5]]
    try:
        from scipy.special import expit, softmax
    except ImportError:
        return
    scores = rng.standard_normal((50, 5)) * 5
    assert np.max(np.abs(expit(scores[:, 0]) - forest_ref.boosted_proba_ld(scores[:, :1])[:, 1])) <= 1e-15
    assert np.max(np.abs(softmax(scores, axis=1) - forest_ref.boosted_proba_ld(scores))) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- HMM
def test_hmm_longdouble_restatements_agree_with_fp64():
    for K, D in ((1, 1), (3, 7), (8, 9), (17, 256)):
        model = hmm_ref.synthetic_model(K, D, 5 + K)
        X = hmm_ref.synthetic_sequence(model, 90, 6)
        B, Bl = hmm_ref.log_likelihood(X, model[2], model[3]), hmm_ref.log_likelihood_ld(X, model[2], model[3])
        assert np.max(np.abs(B - Bl) / np.maximum(np.abs(Bl), 1)) <= 1e-13
        lp = hmm_ref.viterbi(model[0], model[1], B)[0]
        assert abs(lp - hmm_ref.logprob_ld(model[0], model[1], Bl)) <= 1e-12 * abs(lp)
    rng = np.random.default_rng(2)
    F = rng.standard_normal((6, 400)) * 2 + 3
    labels = rng.integers(0, 4, 400)
    want = hmm_ref.train_statistics(F, labels)
    for dtype in (np.float64, np.longdouble):
        got = hmm_ref.train_statistics_k(F, labels, 4, dtype)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.max(np.abs(got[2] - want[2])) <= 1e-13 and np.max(np.abs(got[3] - want[3])) <= 1e-13
    got = hmm_ref.train_statistics_k(F, np.where(labels == 3, 0, labels), 5)
    assert np.isnan(got[2][3:]).all() and np.isnan(got[1][3:]).all() and np.all(got[0][3:] == 0)
    try:
        from scipy.stats import multivariate_normal
    except ImportError:
        return
    model = hmm_ref.synthetic_model(3, 7, 8)
    X = hmm_ref.synthetic_sequence(model, 40, 6)
    for k in range(3):
        ref = multivariate_normal(model[2][k], np.diag(model[3][k])).logpdf(X)
        assert np.max(np.abs(ref - hmm_ref.log_likelihood_ld(X, model[2], model[3])[:, k])) <= 1e-11


@pytest.mark.parametrize("case", range(len(hmm_ref.TWIN_CASES)))
def test_hmm_twin_cases_tie_across_seams_and_nowhere_else(case):
    K, D, twins, seed = hmm_ref.TWIN_CASES[case]
    kp = 2
    while kp < K:
        kp *= 2
    assert kp == (2, 4, 8, 16, 32, 32)[case]
    for T in hmm_ref.TWIN_T:
        model, twins, X = hmm_ref.twin_case(case, T)
        start, trans, means, covars = model
        for a, b in twins:
            assert np.array_equal(means[a], means[b]) and np.array_equal(covars[a], covars[b]) and start[a] == start[b]
            assert np.array_equal(trans[a], trans[b]) and np.array_equal(trans[:, a], trans[:, b])
        B = hmm_ref.log_likelihood(X, means, covars)
        lp, states, margins, reduced = hmm_ref.viterbi_twins(start, trans, B, twins)
        assert reduced.min() >= MIN_MARGIN, (case, T, reduced.min())             # nothing is excluded on the device
        tied = margins == 0
        assert np.array_equal(tied, np.isin(states, [a for a, _ in twins]))        # the ties are the twins', all of them
        assert not np.isin(states, hmm_ref.higher_twins(twins)).any()
        if T >= 257:
            for L in hmm_ref.BLOCK_ROWS:
                seams = range(L, T, L)
                assert not len(seams) or any(tied[t - 1] and tied[t] for t in seams), (case, T, L)


def test_hmm_segment_ragged_and_impossible_cases_clear_the_margin():
    """The margin conditions of the remaining sequences of tests/test_hmm_edges_gpu.py, from the reference alone."""
    for case, T, L in hmm_ref.SEGMENT_CASES:
        model, twins, X = hmm_ref.segment_case(case, T)
        assert X.shape[0] == T and (T + L - 1) // L > 64
        B = hmm_ref.log_likelihood(X, model[2], model[3])
        _, states, margins, reduced = hmm_ref.viterbi_twins(model[0], model[1], B, twins)
        assert reduced.min() >= MIN_MARGIN, (case, T, reduced.min())
        assert np.count_nonzero(margins == 0) >= T // 4 and not np.isin(states, hmm_ref.higher_twins(twins)).any()
        assert reduced[:1].min() >= MIN_MARGIN or T == 1
    model, twins, parts = hmm_ref.ragged_parts()
    assert sorted(p.shape[0] for p in parts) == [1, 1, 1, 2, 9, 257, 513]
    for p in parts:
        B = hmm_ref.log_likelihood(p, model[2], model[3])
        assert hmm_ref.viterbi_twins(model[0], model[1], B, twins)[3].min() >= MIN_MARGIN
    model, X, lengths = hmm_ref.impossible_batch()
    with np.errstate(over="ignore", invalid="ignore"):
        B = hmm_ref.log_likelihood(X, model[2], model[3])
        assert np.isneginf(B[31]).all() and np.isneginf(B[41]).all() and np.isfinite(np.delete(B, [31, 41], axis=0)).all()
        pos = 0
        for q, n in enumerate(lengths):
            lp, states, margins = hmm_ref.viterbi(model[0], model[1], B[pos:pos + n])
            assert np.isneginf(lp) == (q in (1, 3))
            real = np.isfinite(margins) & (margins > 0)              # what is left are ties at -inf: index 0 by the rule
            assert not real.any() or margins[real].min() >= MIN_MARGIN
            if q == 1:
                assert np.all(states[11:] == 0) and np.all(margins[11:] == 0) and real[:11].all()
            pos += n


def test_hmm_offset_rows_are_ill_conditioned_for_the_gate():
    F = hmm_ref.offset_rows(700, 3)
    labels = (np.arange(700) // 9) % 3
    ld = hmm_ref.train_statistics_k(F, labels, 3, np.longdouble)
    f64 = hmm_ref.train_statistics_k(F, labels, 3, np.float64)
    assert np.all(np.abs(ld[3][:, 0] - 1e-6) < 2e-7)
    rel = np.abs(f64[3][:, 0] - ld[3][:, 0]) / ld[3][:, 0]
    assert 1e-9 < rel.max() < 1e-2                         # far above 1e-9 relative, invisible to a gate against max(|ref|, 1)


# -------------------------------------------------------------------------------------------------------- diarization
def test_diar_precision_generic_restatements():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((9, 150)) * rng.uniform(0.5, 5, 9)[:, None] + rng.standard_normal(9)[:, None]
    Z, mean, var, scale = diar_ref.standardize(X)
    for dtype in (np.float64, np.longdouble):
        m, v, s, c, _ = diar_ref.standardize_p(X, dtype)
        assert not c.any() and np.max(np.abs(m - mean)) <= 1e-14 and np.max(np.abs(v / var - 1)) <= 1e-13
        assert np.max(np.abs(s / scale - 1)) <= 1e-13
    labels = rng.integers(0, 4, 150)
    S64, Sld = diar_ref.pair_sums_p(Z, labels, 5, np.float64), diar_ref.pair_sums_p(Z, labels, 5)
    assert np.max(np.abs(S64 - Sld) / np.maximum(np.abs(Sld), 1)) <= 1e-12 and np.all(Sld[4] == 0)
    c64, p64 = diar_ref.dim_distances_p(Z, labels == 1, np.float64)
    cld, pld = diar_ref.dim_distances_p(Z, labels == 1)
    assert np.max(np.abs(c64 - cld) / cld) <= 1e-13 and abs(p64 - pld) <= 1e-13 * pld
    init = Z[:4]
    a, b = diar_ref.kmeans(Z, 4, init), diar_ref.kmeans(Z, 4, init, dtype=np.longdouble)
    assert a["margin"] >= DIST_FLOOR and np.array_equal(a["labels"], b["labels"]) and a["n_iter"] == b["n_iter"]
    assert np.max(np.abs(a["centers"] - b["centers"])) <= 1e-13 and abs(a["inertia"] - b["inertia"]) <= 1e-12 * a["inertia"]
    if diar_ref.distance is not None:
        assert np.max(np.abs(diar_ref.pair_sums(Z, labels, 5) - Sld) / np.maximum(np.abs(Sld), 1)) <= 1e-12
        kept, s, margin = diar_ref.kept_dimensions(Z)
        assert np.max(np.abs(s - diar_ref.dim_distances_p(Z)[0]) / s) <= 1e-13


def test_diar_hand_labels_hold_the_promised_clusters():
    for n in (127, 128, 129, 255, 256, 257):
        L = diar_ref.hand_labels(n)
        for lab, k in zip(L, diar_ref.PAIR_KS):
            cnt = np.bincount(lab, minlength=k)
            assert lab.min() >= 0 and lab.max() < k and cnt[1] == 1 and lab[n - 1] == 1
            if k > 2:
                assert cnt[k - 1] == 0
            if k >= 5:
                assert np.array_equal(np.flatnonzero(lab == 2), np.arange(3, 14))
            assert np.count_nonzero(cnt) >= min(k, 3) - 1


def test_diar_scaler_rows_are_clear_of_the_constant_bound():
    for n in (255, 256, 257, 300):
        X, constant = diar_ref.scaler_rows(n)
        for dtype in (np.float64, np.longdouble):
            m, v, s, c, bound = diar_ref.standardize_p(X, dtype)
            assert np.array_equal(c, constant), (n, dtype)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.asarray(v / bound, dtype=np.float64)
            live = v > 0
            assert np.all((ratio[live] > 1e3) | (ratio[live] < 1e-3)), ratio        # no decision near the bound


def test_diar_kmeans_designs_are_exact():
    for lead in (0, 1, 6):
        Z, init = diar_ref.equidistant_case(lead)
        k = init.shape[0]
        d2 = diar_ref.sq_distances(Z, init)
        tied = Z[:, 1] == 4.0
        assert tied.sum() == 64 and np.all(d2[tied, lead] == d2[tied, lead + 1]) and np.all(d2[tied, lead] == d2[tied].min(axis=1))
        assert len({int(i) // 256 for i in np.flatnonzero(tied)}) >= 2              # in several assign workgroups
        a, b = diar_ref.kmeans(Z, k, init), diar_ref.kmeans(Z, k, init, dtype=np.longdouble)
        assert a["n_iter"] == b["n_iter"] == 2 and a["strict"] and a["margin"] == 0.0
        assert np.array_equal(a["labels"], b["labels"]) and np.all(a["labels"][tied] == lead)
        assert np.array_equal(a["centers"], b["centers"].astype(np.float64)) and np.all(b["centers"] == b["centers"].astype(np.float64))
        assert a["inertia"] == float(b["inertia"]) == 960.0
    Z, init = diar_ref.two_empty_case()
    d2 = diar_ref.sq_distances(Z, init)
    assert set(np.argmin(d2, axis=1)) == {0, 1}
    near = d2.min(axis=1)
    assert sorted(np.flatnonzero(near == near.max())) == sorted(diar_ref.FAR_TIES) and near.max() == 36.0
    assert len({tuple(p) for p in diar_ref.FAR_TIES.values()}) == 3
    a, b = diar_ref.kmeans(Z, 4, init, max_iter=1), diar_ref.kmeans(Z, 4, init, max_iter=1, dtype=np.longdouble)
    assert a["centers"][2].tolist() == [0.0, 6.0] and a["centers"][3].tolist() == [0.0, -6.0]
    assert np.array_equal(a["centers"], b["centers"].astype(np.float64)) and np.all(b["centers"] == b["centers"].astype(np.float64))
    assert a["inertia"] == float(b["inertia"]) and np.array_equal(a["labels"], b["labels"])
    full, full_ld = diar_ref.kmeans(Z, 4, init), diar_ref.kmeans(Z, 4, init, dtype=np.longdouble)
    assert np.array_equal(full["labels"], full_ld["labels"]) and full["n_iter"] == full_ld["n_iter"]


def test_diar_stage_and_near_duplicate_cases():
    X, inits = diar_ref.stage_case()
    assert X.shape == (17, 257)
    mean, var, scale, constant, _ = diar_ref.standardize_p(X)
    Z = ((np.asarray(X, dtype=np.longdouble) - mean[:, None]) / scale[:, None]).T
    colsum, _ = diar_ref.dim_distances_p(Z)
    m = colsum.mean()
    assert not constant.any() and float(np.min(np.abs(colsum - 1.1 * m)) / m) >= DIST_FLOOR
    kept = np.nonzero(colsum < 1.1 * m)[0]
    assert 1 <= kept.shape[0] < 17 and inits.shape == (3, kept.shape[0])
    for dtype in (np.float64, np.longdouble):
        r = diar_ref.kmeans(np.asarray(Z[:, kept], dtype=dtype), 3, inits, dtype=dtype)
        assert r["margin"] >= DIST_FLOOR and np.bincount(r["labels"], minlength=3).min() > 0
    X, labels = diar_ref.near_duplicate_case()
    ld, f64 = diar_ref.pair_sums_p(X.T, labels, 3), diar_ref.pair_sums_p(X.T, labels, 3, np.float64)
    assert 0 < ld[2, 2] < 1e-4 and ld[0, 0] > 1e3
    assert abs(f64[2, 2] - ld[2, 2]) / ld[2, 2] < 1e-12            # the difference form keeps even this sum accurate
