"""The references of the similarity / thumbnail / onset-SVM edge suites checked on the CPU: tests/sim_ref.py against SciPy,
scikit-learn and the float64 oracle, tests/onset_svm_ref.py against SVC.predict_proba, and every input generator of
tests/test_similarity_edges_gpu.py and tests/test_onset_svm_edges_gpu.py run once with the properties asserted that the
GPU tests rely on (NaN patterns, tie counts, decision margins, distance from the early-exit threshold) -- a GPU failure
cannot be the generator's fault.  SciPy / scikit-learn are imported per test: these are tests of the reference, not of
a kernel."""
import numpy as np
import pytest

import onset_svm_ref as R
import paa_oracle as O
import sim_ref
import svc_libsvm


# ---------------------------------------------------------------------------------------------------------
# sim_ref against SciPy / scikit-learn / the float64 oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,n", [(68, 300), (5, 40), (1, 37), (13, 129)])
def test_similarity_reference_matches_scipy_and_oracle(dims, n):
    distance = pytest.importorskip("scipy.spatial.distance")
    preprocessing = pytest.importorskip("sklearn.preprocessing")
    F = sim_ref.seeded_features(dims, n)
    if dims > 4:
        F[3] = 2.5                                        # constant row: scale 1
    ref = np.asarray(sim_ref.self_similarity(F), dtype=np.float64)
    Z = preprocessing.StandardScaler().fit_transform(F.T)
    sp = 1.0 - distance.squareform(distance.pdist(Z, "cosine"))
    assert np.max(np.abs(ref - sp)) <= 1e-12
    assert np.max(np.abs(ref - O.self_similarity_matrix(F))) <= 1e-12
    assert np.max(np.abs(np.asarray(sim_ref.standardize_rows(F), dtype=np.float64) - Z.T)) <= 1e-10
    f64 = sim_ref.self_similarity(F, dtype=np.float64)
    assert np.array_equal(np.diag(f64), np.ones(n)) and np.max(np.abs(f64 - ref)) <= 1e-12


@pytest.mark.parametrize("n,M,band,l1,l2", [(60, 7, 10.0, 0, 1), (45, 1, 2.0, 0.1, 0.9), (33, 33, 10.0, 0, 1),
                                            (50, 20, 0.5, 0.3, 0.7)])
def test_thumbnail_reference_matches_convolve2d(n, M, band, l1, l2):
    signal = pytest.importorskip("scipy.signal")
    S = O.self_similarity_matrix(np.random.default_rng(n).standard_normal((12, n)).cumsum(axis=1))
    sm = signal.convolve2d(S, np.eye(M), "valid")
    min_sm = np.min(sm)
    for i in range(sm.shape[0]):                          # audioSegmentation.py:1149-1160, with band = 5.0 / short_step
        for j in range(sm.shape[1]):
            if abs(i - j) < band or i > j:
                sm[i, j] = min_sm
    sm[0:int(l1 * sm.shape[0]), :] = min_sm
    sm[:, 0:int(l1 * sm.shape[0])] = min_sm
    sm[int(l2 * sm.shape[0])::, :] = min_sm
    sm[:, int(l2 * sm.shape[0])::] = min_sm
    ref = sim_ref.thumbnail_filter(S, M, band, l1, l2)
    assert np.max(np.abs(np.asarray(ref, dtype=np.float64) - sm)) <= 1e-12 * M
    pos, _ = sim_ref.argmax_margin(ref)
    f64 = sim_ref.thumbnail_filter(S, M, band, l1, l2, dtype=np.float64)
    if sim_ref.argmax_margin(f64)[1] > 1e-9:
        assert pos == tuple(int(v) for v in np.unravel_index(np.argmax(sm), sm.shape))
    assert np.all(sm[sim_ref.mask(sm.shape[0], band, l1, l2)] == min_sm)
    assert np.max(np.abs(f64 - O.thumbnail_filter(S, M, 5.0 / band, l1, l2))) <= 1e-12 * M


def test_argmax_margin_helper():
    a = np.array([[1.0, 3.0, 3.0], [2.5, 3.0, 0.0]])
    assert sim_ref.argmax_margin(a) == ((0, 1), 0.5)
    assert sim_ref.argmax_margin(np.full((2, 2), 4.0)) == ((0, 0), float("inf"))
    a[1, 0] = np.nan
    pos, margin = sim_ref.argmax_margin(a)
    assert pos == (1, 0) and np.isnan(margin)
    assert sim_ref.same_bits(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0]))
    assert not sim_ref.same_bits(np.array([0.0]), np.array([-0.0]))
    assert sim_ref.untouched(np.full(3, sim_ref.SENTINEL)) and not sim_ref.untouched(np.array([sim_ref.SENTINEL, 0.0]))


# ---------------------------------------------------------------------------------------------------------
# generators of tests/test_similarity_edges_gpu.py
# ---------------------------------------------------------------------------------------------------------
def test_shape_cases_cover_both_axes():
    cases = sim_ref.sim_shape_cases()
    big, tiles = sim_ref.persistent_n_vec()
    assert tiles * (tiles + 1) // 2 > 512 and (tiles - 1) * tiles // 2 <= 512 and -(-big // 128) == tiles
    assert big % 128 not in (0, 1, 127)
    assert {n for n, _ in cases} == set(sim_ref.SIM_N_VEC) | {big}
    assert {d for _, d in cases} == set(sim_ref.SIM_N_DIMS)
    for n in sim_ref.SIM_N_VEC:
        assert len({d for m, d in cases if m == n}) == 3
    for d in sim_ref.SIM_N_DIMS:
        assert len({n for n, m in cases if m == d}) >= 3
    assert len(cases) == len(set(cases)) == 35


def test_exact_zero_features_nan_pattern():
    F, zc = sim_ref.exact_zero_features(12, 200, (5, 127, 128, 199))
    assert zc == [5, 127, 128, 199, 205, 327, 328, 399]
    assert np.all(F.sum(axis=1) == 0.0) and np.array_equal(F, np.round(F))
    ref = np.asarray(sim_ref.self_similarity(F), dtype=np.float64)
    expect = np.zeros(ref.shape, dtype=bool)
    expect[zc, :] = True
    expect[:, zc] = True
    np.fill_diagonal(expect, False)
    assert np.array_equal(np.isnan(ref), expect)
    assert np.array_equal(np.isnan(O.self_similarity_matrix(F)), expect)
    assert np.all(np.diag(ref) == 1.0)


def test_duplicate_features_are_plus_minus_one():
    for q in (1, 33, 100):
        F, pairs = sim_ref.duplicate_features(9, q, seed=q)
        assert np.all(F.sum(axis=1) == 0.0)
        ref = sim_ref.self_similarity(F)
        for i, j, sign in pairs:
            assert abs(float(ref[i, j]) - sign) <= 1e-18, (q, i, j)


def test_conditioning_cases_are_what_they_claim():
    for case, ratio in zip(sim_ref.CONDITIONING_CASES[:3], (1e3, 1e6, 1e9)):
        F = sim_ref.conditioning_features(case)
        assert F.shape == (20, 300)
        r = np.abs(F.mean(axis=1)) / F.std(axis=1)
        assert np.all(r > 0.8 * ratio) and np.all(r < 1.3 * ratio)
    F = sim_ref.conditioning_features("near_constant")
    mean, var, bound, rounding = sim_ref.row_stats(F)
    # no row's classification depends on float64 rounding: the either-classification clause admits 0 cases
    assert np.all(np.abs(var - bound) > rounding)
    constant = var <= bound
    assert constant[9] and not constant[5] and constant.sum() == 1
    assert 100 < float(np.sqrt(var[5])) / (300 * sim_ref.EPS) < 1e4
    assert 0.01 < float(np.sqrt(var[9])) / (300 * sim_ref.EPS) < 1.0
    m64, v64, b64, _ = sim_ref.row_stats(F, dtype=np.float64)
    assert np.array_equal(v64 <= b64, constant)


def test_oracle_error_against_longdouble_grows_with_the_offset():
    """The float64 oracle is 1e-13 / 1e-10 / 1e-7 away from the longdouble restatement at mean / sigma of 1e3 / 1e6 / 1e9:
    a fixed 1e-9 is the wrong yardstick there."""
    errs = []
    for case in sim_ref.CONDITIONING_CASES[:3]:
        F = sim_ref.conditioning_features(case)
        errs.append(float(np.max(np.abs(O.self_similarity_matrix(F) - sim_ref.self_similarity(F)))))
    assert errs[0] < 1e-11 and errs[0] < errs[1] < errs[2] and errs[2] > 1e-9


def test_dyadic_matrices_give_exact_window_sums():
    for n, M in ((64, 32), (287, 33)):
        S = sim_ref.dyadic_matrix(n, seed=n)
        assert np.array_equal(S, S.T) and np.array_equal(S * 8, np.round(S * 8)) and np.abs(S).max() <= 1.0
        assert not np.any(np.signbit(S) & (S == 0))
        ld = sim_ref.window_sums(S, M)
        f64 = sim_ref.window_sums(S, M, dtype=np.float64)
        assert np.array_equal(np.asarray(ld, dtype=np.float64), f64) and np.array_equal(f64 * 8, np.round(f64 * 8))
    sizes = {n - M + 1 for n, M in sim_ref.THUMB_SIZES}
    assert sizes == {1, 2, 31, 32, 33, 255, 256, 257, 1023, 1025, 2049}
    assert {M for _, M in sim_ref.THUMB_SIZES} == {1, 2, 31, 32, 33, 64, 40}


def test_tied_matrix_spreads_its_maxima():
    S = sim_ref.tied_matrix(600)
    assert np.array_equal(S, S.T) and set(np.unique(S)) <= {0.0, 0.5, 1.0}
    filt = np.asarray(sim_ref.thumbnail_filter(S, 7, 10.0, 0, 1), dtype=np.float64)
    count, xblocks, yblocks, waves = sim_ref.tie_spread(filt)
    assert count >= 8 and xblocks >= 2 and yblocks >= 2 and waves >= 2, (count, xblocks, yblocks, waves)
    assert filt.max() > filt.min()


def test_truncation_cases_straddle_integers():
    below = at = 0
    for Rr, l1, l2 in sim_ref.THUMB_TRUNC:
        for lim in (l1, l2):
            prod = lim * Rr
            exact = round(lim * 100) * Rr / 100.0
            assert exact == int(exact)
            below += int(prod) < exact
            at += int(prod) == exact
    assert below >= 2 and at >= 2


def test_degenerate_matrices_reach_the_fill_value():
    n, M, band = 70, 5, 6.0
    mats = sim_ref.degenerate_matrices(n, band)
    for name, S in mats.items():
        assert np.array_equal(S, S.T)
        sums = sim_ref.window_sums(S, M, dtype=np.float64)
        filt = sim_ref.thumbnail_filter(S, M, band, 0, 1, dtype=np.float64)
        unmasked = ~sim_ref.mask(n - M + 1, band, 0, 1)
        assert unmasked.any() and filt[unmasked].max() == sums.min(), name
    assert sim_ref.window_sums(mats["max_is_min"], M, dtype=np.float64).max() > sums.min()
    assert sim_ref.mask(66, 71.0, 0, 1).all() and sim_ref.mask(66, 3.0, 0.9, 0.1).all()
    assert not sim_ref.mask(66, 0.0, 0, 1)[0, 0] and sim_ref.mask(66, 0.5, 0, 1)[0, 0]


def test_nan_matrices_forget_the_nan_after_the_window():
    n = 200
    for M in sim_ref.THUMB_NAN_M:
        R = n - M + 1
        for name, S in sim_ref.nan_matrices(n, seed=3).items():
            sums = np.asarray(sim_ref.window_sums(S, M), dtype=np.float64)
            nan = np.isnan(sums)
            if name in ("run_start", "mid_run", "run_end"):
                a = {"run_start": 64, "mid_run": 80, "run_end": 95}[name]
                expect = np.zeros((R, R), dtype=bool)
                for k in range(M):
                    for i, j in ((a - k, a + 50 - k), (a + 50 - k, a - k)):
                        if 0 <= i < R and 0 <= j < R:
                            expect[i, j] = True
                assert np.array_equal(nan, expect) and nan.sum() == 2 * M
            elif name == "row_and_column":
                assert nan.any() and not nan.all() and not nan[80 + M:, 80 + M:].any()
            else:
                assert nan.all()
            filt = sim_ref.thumbnail_filter(S, M, 3.0, 0, 1)
            pos, margin = sim_ref.argmax_margin(filt)
            assert np.isnan(margin) and pos == (0, 0)          # the fill value is NaN: first masked cell


@pytest.mark.parametrize("n_vec", [1151, 3001])
def test_feature_clips_have_a_clear_argmax(n_vec):
    M = 20
    F = sim_ref.clip_features(n_vec, seed=n_vec)
    filt = sim_ref.thumbnail_filter(O.self_similarity_matrix(F), M, 10.0, 0, 1, dtype=np.float64)
    pos, margin = sim_ref.argmax_margin(filt)
    assert margin > 100 * 1e-9 * M, margin
    assert pos[1] - pos[0] >= 10 and not np.isnan(filt).any()


# ---------------------------------------------------------------------------------------------------------
# onset_svm_ref
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_onset_reference_equals_predict_proba(kernel):
    sklearn_svm = pytest.importorskip("sklearn.svm")
    rng = np.random.default_rng(5)
    n_dims = 12
    X = np.vstack([rng.standard_normal((80, n_dims)) - 0.7, rng.standard_normal((80, n_dims)) + 0.7])
    y = np.append(np.zeros(80), np.ones(80))
    np.random.seed(3)
    svm = sklearn_svm.SVC(C=1.0, kernel=kernel, probability=True, gamma="auto", random_state=7).fit(X, y)
    model = {"sv": np.ascontiguousarray(svm.support_vectors_), "coef": np.ascontiguousarray(svm.dual_coef_.reshape(-1)),
             "intercept": float(svm.intercept_[0]), "gamma": float(svm._gamma) if kernel == "rbf" else 0.0,
             "prob_a": float(svm.probA_[0]), "prob_b": float(svm.probB_[0])}
    mean, scale = rng.uniform(-1, 1, n_dims), rng.uniform(0.5, 2, n_dims)
    frames = rng.standard_normal((300, n_dims)) * 1.5
    feats = np.ascontiguousarray((frames * scale + mean).T)
    got = R.predict(model, feats, mean, scale)
    Xs = ((feats - mean[:, None]) / scale[:, None]).T
    ref = svm.predict_proba(Xs)[:, 1]
    assert np.max(np.abs(got["prob1"] - ref)) < 1e-10
    assert np.max(np.abs(R.decision_function(model, Xs) - svm.decision_function(Xs))) < 1e-12
    # the same numbers through the multi-class restatement the SVC suite uses
    full = svc_libsvm.predict(svc_libsvm.model_arrays(svm), Xs)[1][:, 1]
    assert np.max(np.abs(got["prob1"] - full)) < 1e-13


def test_two_class_iteration_equals_the_general_restatement():
    r01 = np.concatenate([[1e-7, 1 - 1e-7, 0.5, 0.25], np.random.default_rng(1).uniform(1e-7, 1 - 1e-7, 200)])
    got, iters, margin = R.two_class_prob1(r01)
    for v, g in zip(r01, got):
        assert svc_libsvm.multiclass_probability(np.array([[0.0, v], [1.0 - v, 0.0]]))[1] == g
    assert iters[2] == 0 and iters.max() > 1 and np.all(margin >= 0)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_onset_cases_keep_clear_of_the_early_exit(name):
    model, feats, mean, scale, ref, seed = R.make_case(name)
    n_dims, n_frames, n_sv = R.CASES[name][:3]
    assert feats.shape == (n_dims, n_frames) and model["sv"].shape == (n_sv, n_dims)
    assert ref["margin"].min() > R.MARGIN_MIN
    assert np.all(np.isfinite(ref["prob1"])) and np.all((ref["prob1"] > 0) & (ref["prob1"] < 1))
    if name.startswith("sat_"):
        f = ref["fApB"]
        for sign in (1, -1):
            assert np.any(sign * f > 750) and np.any((sign * f > 40) & (sign * f < 700)), (name, sign)
        assert np.any(ref["r01"] == R.CLIP) and np.any(ref["r01"] == 1 - R.CLIP)
        assert np.any((ref["r01"] > R.CLIP) & (ref["r01"] < 1 - R.CLIP))
    elif n_frames >= 63:
        # (gamma = 1e-6 makes every kernel value 1 - O(1e-4): the probabilities still differ by far more than 1e-10)
        assert np.ptp(ref["prob1"]) > (1e-4 if R.CASES[name][3] == 1e-6 else 0.05), "every frame has the same probability"
    if name.startswith("lin_") and n_frames >= 63:
        assert np.any(ref["fApB"] > 0) and np.any(ref["fApB"] < 0)


def test_onset_cases_cover_the_issue_grid():
    dims = {c[0] for c in R.CASES.values()}
    frames = {c[1] for c in R.CASES.values()}
    svs = {c[2] for c in R.CASES.values()}
    assert dims >= {1, 2, 34, 68, 71, 72} and frames >= {1, 63, 64, 255, 256, 257, 1000} and svs >= {1, 2, 97}
    rbf = {c[3] for c in R.CASES.values() if c[3] != 0.0}
    assert rbf >= {1e-6, None, 10.0}
    assert any(c[3] == 0.0 and c[2] > 1 for c in R.CASES.values())
    assert {np.sign(c[4]) for c in R.CASES.values()} == {-1.0, 1.0}
    assert any(c[5] for c in R.CASES.values())
