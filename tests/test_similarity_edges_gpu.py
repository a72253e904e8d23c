"""Edges of the similarity / thumbnail kernels (pyaudioanalysis_amd/csrc/kernels_sim.hpp) against tests/sim_ref.py.  -m gpu.

Similarity stage: tile boundaries (n_vec on and around multiples of 128), the % 4 / 32-row chunk boundaries of n_dims, a
size whose tile triangle exceeds two tiles per compute unit (persistent workgroups take a second and third tile), leading
dimensions above n_vec with NaN padding, sentinel / guard-band checks of the output, exact NaN and +-1 structure, and
badly conditioned rows judged against an np.longdouble reference with the float64 oracle's own error as the yardstick.
Thumbnail stage alone: matrices of multiples of 1/8, for which every window sum and sliding update is exact -- the
filtered matrix must equal the reference bit for bit and the arg-max must be identical, ties, degenerate maxima and NaN
included.  Every generator's promised properties are asserted on the CPU in tests/test_sim_ref_cpu.py.

The whole file (104 cases with tests/test_onset_svm_edges_gpu.py) took 11 s on one MI355X, library load included."""
import numpy as np
import pytest

import paa_oracle as O
import sim_ref
from pyaudioanalysis_amd import _ffi

pytestmark = pytest.mark.gpu

# Conditioning: the kernel may be K_COND x as far from the longdouble reference as the float64 oracle is, plus a floor of
# 4e-16.  K_COND is the smallest power of two that is at least twice the largest ratio recorded in
# profiles/r07_sim_edge_errors.json.
K_COND = 4
COND_FLOOR = 4e-16


def _similarity(lib, F, ld=None):
    rc, S, guard = sim_ref.dev_self_similarity(lib, F, ld)
    assert rc == 0, _ffi.last_error()
    assert not np.any(S == sim_ref.SENTINEL), "%d output elements were never written" % np.sum(S == sim_ref.SENTINEL)
    assert sim_ref.untouched(guard), "the guard band after the output was written"
    return S


def _check_invariants(S):
    n = S.shape[0]
    assert sim_ref.same_bits(S, S.T), "not bitwise symmetric"
    assert np.array_equal(np.diag(S), np.ones(n)), "diagonal is not exactly 1"
    assert np.all(np.abs(S[~np.isnan(S)]) <= 1.0)


def _cmp_nan(got, ref, tol, what):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN pattern differs"
    d = np.abs(np.nan_to_num(got) - np.nan_to_num(ref))
    print("%s: max abs diff %.3g" % (what, d.max()))
    assert d.max() <= tol, "%s: max abs diff %g > %g" % (what, d.max(), tol)


# ---------------------------------------------------------------------------------------------------------
# similarity stage
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vec,n_dims", sim_ref.sim_shape_cases())
def test_similarity_shapes_strides_bounds(gpu_lib, n_vec, n_dims):
    F = sim_ref.seeded_features(n_dims, n_vec)
    if n_dims > 4:
        F[3] = 2.5                                          # constant row: scale 1
    S = _similarity(gpu_lib, F)
    _check_invariants(S)
    if n_vec > 1:
        assert not np.isnan(S).any()
    _cmp_nan(S, O.self_similarity_matrix(F), 1e-9, "sim %d x %d" % (n_dims, n_vec))
    assert sim_ref.same_bits(S, _similarity(gpu_lib, F)), "two calls differ"
    for ld in (n_vec + 1, n_vec + 129):
        assert sim_ref.same_bits(S, _similarity(gpu_lib, F, ld)), "ld = n_vec + %d changes the result" % (ld - n_vec)
    # the host wrapper takes the same path
    from pyaudioanalysis_amd import audioSegmentation
    assert sim_ref.same_bits(S, audioSegmentation.self_similarity_matrix(F))


def test_similarity_ignores_stale_scratch(gpu_lib):
    """The standardised matrix lives in a scratch buffer shared by all calls, padded to a multiple of 4 rows and 128
    columns: the padding is rewritten on every call, so a result does not depend on what an earlier call left there."""
    small, large = sim_ref.seeded_features(5, 129), sim_ref.seeded_features(68, 1151)
    s0 = _similarity(gpu_lib, small)
    l0 = _similarity(gpu_lib, large)
    assert sim_ref.same_bits(s0, _similarity(gpu_lib, small)), "small shape after a large call"
    assert sim_ref.same_bits(l0, _similarity(gpu_lib, large)), "large shape after a small call"
    other = sim_ref.seeded_features(33, 257, seed=1)
    o0 = _similarity(gpu_lib, other)
    _similarity(gpu_lib, np.full((136, 1151), 3.0) + sim_ref.seeded_features(136, 1151))
    assert sim_ref.same_bits(o0, _similarity(gpu_lib, other))
    _cmp_nan(o0, O.self_similarity_matrix(other), 1e-9, "33 x 257")


@pytest.mark.parametrize("half,zero_cols", [(200, (5, 127, 128, 199)), (64, (0, 63)), (576, (127, 128, 300, 575))])
def test_similarity_zero_vectors_give_exactly_their_rows_and_columns(gpu_lib, half, zero_cols):
    F, zc = sim_ref.exact_zero_features(12, half, zero_cols, seed=half)
    S = _similarity(gpu_lib, F)
    _check_invariants(S)
    expect = np.zeros(S.shape, dtype=bool)
    expect[zc, :] = True
    expect[:, zc] = True
    np.fill_diagonal(expect, False)
    assert np.array_equal(np.isnan(S), expect)
    _cmp_nan(S, O.self_similarity_matrix(F), 1e-9, "zero vectors")
    assert sim_ref.same_bits(S, _similarity(gpu_lib, F, 2 * half + 129))


@pytest.mark.parametrize("quarter", [1, 33, 100, 288])
def test_similarity_duplicates_are_plus_minus_one(gpu_lib, quarter):
    F, pairs = sim_ref.duplicate_features(9, quarter, seed=quarter)
    S = _similarity(gpu_lib, F)
    _check_invariants(S)
    ulp = np.finfo(np.float64).eps
    for i, j, sign in pairs:
        assert abs(S[i, j]) <= 1.0 and abs(S[i, j] - sign) <= 2 * ulp, (i, j, sign, S[i, j])
    _cmp_nan(S, O.self_similarity_matrix(F), 1e-9, "duplicates")


@pytest.mark.parametrize("case", sim_ref.CONDITIONING_CASES)
def test_similarity_conditioning_against_longdouble(gpu_lib, case):
    """Rows with mean / sigma of 1e3, 1e6, 1e9 and near-constant rows: the float64 oracle itself is up to 1.7e-7 away
    from the longdouble restatement, so the kernel is held to K_COND x the oracle's own error + 4e-16.
    The either-classification clause for near-constant rows admits 0 cases: both planted rows (5: not constant, 9:
    constant) are further from the rule's threshold than float64 rounding can move them (asserted on the CPU), so the
    kernel's classification must be the reference's."""
    F = sim_ref.conditioning_features(case)
    ref = sim_ref.self_similarity(F)
    S = _similarity(gpu_lib, F)
    _check_invariants(S)
    err_kernel = float(np.max(np.abs(S - ref)))
    err_oracle = float(np.max(np.abs(O.self_similarity_matrix(F) - ref)))
    print("conditioning %s: kernel %.3g oracle %.3g ratio %.3g" % (case, err_kernel, err_oracle, err_kernel / err_oracle))
    assert err_kernel <= K_COND * err_oracle + COND_FLOOR, (case, err_kernel, err_oracle)


def test_similarity_argument_errors(gpu_lib):
    d = _ffi.DeviceBuffer.from_host(np.full(64, sim_ref.SENTINEL))
    try:
        for args in ((None, 2, 4, 4, d.ptr), (d.ptr, 2, 4, 4, None), (d.ptr, 0, 4, 4, d.ptr), (d.ptr, 2, 0, 4, d.ptr),
                     (d.ptr, 2, 4, 3, d.ptr)):
            assert gpu_lib.paa_dev_self_similarity(*args) == _ffi.ERR_ARG
        _ffi.sync()
        assert sim_ref.untouched(d.to_host(np.float64, 64))
    finally:
        d.free()


# ---------------------------------------------------------------------------------------------------------
# thumbnail stage alone: exact inputs, bit-for-bit results
# ---------------------------------------------------------------------------------------------------------
def _thumbnail_exact(lib, S, M, band, l1, l2, what):
    rc, filt, pos, guard = sim_ref.dev_thumbnail_filter(lib, S, M, band, l1, l2)
    assert rc == 0, _ffi.last_error()
    assert not np.any(filt == sim_ref.SENTINEL), what + ": output elements were never written"
    assert sim_ref.untouched(guard), what + ": the guard band after the output was written"
    ref = np.asarray(sim_ref.thumbnail_filter(S, M, band, l1, l2), dtype=np.float64)
    assert np.array_equal(np.isnan(filt), np.isnan(ref)), \
        "%s: NaN pattern differs in %d cells" % (what, np.sum(np.isnan(filt) != np.isnan(ref)))
    assert sim_ref.same_bits(filt, ref), "%s: %d cells differ" % (what, np.sum(np.nan_to_num(filt) != np.nan_to_num(ref)))
    assert pos == sim_ref.argmax_margin(ref)[0], (what, pos, sim_ref.argmax_margin(ref)[0])
    return filt


@pytest.mark.parametrize("n,M", sim_ref.THUMB_SIZES)
def test_thumbnail_sizes_bit_exact(gpu_lib, n, M):
    S = sim_ref.dyadic_matrix(n, seed=n + M)
    for band in (3.0, 10.0):
        _thumbnail_exact(gpu_lib, S, M, band, 0, 1, "n %d M %d band %g" % (n, M, band))
    _thumbnail_exact(gpu_lib, S, M, 0.0, 0.1, 0.9, "n %d M %d band 0" % (n, M))


def test_thumbnail_ties_first_maximum_wins(gpu_lib):
    """Periodic matrix over {0, 1/2, 1}: the maximum occurs in several thumb_diag x blocks, y blocks and waves (asserted
    on the CPU); the first one in row-major order must win."""
    S = sim_ref.tied_matrix(600)
    filt = _thumbnail_exact(gpu_lib, S, 7, 10.0, 0, 1, "ties")
    count, xblocks, yblocks, waves = sim_ref.tie_spread(filt)
    assert count >= 8 and xblocks >= 2 and yblocks >= 2 and waves >= 2
    for band, l1, l2 in ((0.0, 0, 1), (10.0, 0.3, 0.9), (40.0, 0, 0.7), (1.0, 0.05, 1)):
        _thumbnail_exact(gpu_lib, S, 7, band, l1, l2, "ties band %g limits %g %g" % (band, l1, l2))
    _thumbnail_exact(gpu_lib, sim_ref.tied_matrix(1200, period=40), 33, 10.0, 0, 1, "ties 1200")


@pytest.mark.parametrize("band_name", sim_ref.THUMB_BANDS)
def test_thumbnail_masks(gpu_lib, band_name):
    S = sim_ref.dyadic_matrix(110, seed=11)
    R = 100
    for l1, l2 in sim_ref.THUMB_LIMITS:
        _thumbnail_exact(gpu_lib, S, 11, sim_ref.band_value(band_name, R), l1, l2,
                         "band %s limits %g %g" % (band_name, l1, l2))


@pytest.mark.parametrize("R,l1,l2", sim_ref.THUMB_TRUNC)
def test_thumbnail_limit_truncation(gpu_lib, R, l1, l2):
    M = 4
    S = sim_ref.dyadic_matrix(R + M - 1, seed=R)
    for band in (0.0, 2.0):
        _thumbnail_exact(gpu_lib, S, M, band, l1, l2, "R %d limits %g %g band %g" % (R, l1, l2, band))
        _thumbnail_exact(gpu_lib, S, M, band, 0, l1, "R %d limits 0 %g band %g" % (R, l1, band))


@pytest.mark.parametrize("band,l1,l2", [(6.0, 0.2, 1), (6.0, 0, 0.8), (0.0, 0, 1), (0.0, 0.2, 0.8), (6.0, 0, 1)])
def test_thumbnail_degenerate_argmax(gpu_lib, band, l1, l2):
    """The maximum of the masked matrix is the fill value: constant matrix, unmasked maximum equal to the global minimum,
    everything masked.  The expected position is numpy.argmax of the reference's masked matrix."""
    n, M = 70, 5
    for name, S in sim_ref.degenerate_matrices(n, 6.0).items():
        _thumbnail_exact(gpu_lib, S, M, band, l1, l2, name)
    S = sim_ref.dyadic_matrix(n, seed=7)
    _thumbnail_exact(gpu_lib, S, M, 71.0, l1, l2, "everything masked by the band")
    _thumbnail_exact(gpu_lib, S, M, band, 0.9, 0.1, "everything masked by the limits")
    _thumbnail_exact(gpu_lib, S, M, band, 0, 0, "everything masked by limit_2 = 0")


@pytest.mark.parametrize("M", sim_ref.THUMB_NAN_M)
def test_thumbnail_nan(gpu_lib, M):
    """NaN cells at a run start, mid run and run end of thumb_diag's 32-cell diagonal runs, a NaN row and column, all NaN.
    The window forgets a NaN M cells later (direct sums in the reference); a sliding sum that carried it would write NaN
    into cells where the reference is finite."""
    for name, S in sim_ref.nan_matrices(200, seed=3).items():
        for band in (3.0, 0.0):
            _thumbnail_exact(gpu_lib, S, M, band, 0, 1, "NaN %s M %d band %g" % (name, M, band))
        _thumbnail_exact(gpu_lib, S, M, 3.0, 0.1, 0.9, "NaN %s M %d limits" % (name, M))


def test_thumbnail_argument_errors(gpu_lib):
    """Rejected by the host before any launch: the sentinel-filled output is untouched."""
    S = sim_ref.dyadic_matrix(20, seed=1)
    bad = [dict(M=21), dict(M=0), dict(M=-3), dict(M=5, n_vec=0), dict(M=5, n_vec=-1), dict(M=5, n_vec=4),
           dict(M=5, l1=-0.1), dict(M=5, l2=-1.0), dict(M=5, l1=float("nan")), dict(M=5, l2=float("nan")),
           dict(M=5, null="sim"), dict(M=5, null="filt"), dict(M=5, null="pos")]
    for kw in bad:
        rc, filt, pos, guard = sim_ref.dev_thumbnail_filter(gpu_lib, S, kw["M"], 3.0, kw.get("l1", 0.0), kw.get("l2", 1.0),
                                                            null=kw.get("null"), n_vec=kw.get("n_vec"))
        assert rc == _ffi.ERR_ARG, (kw, rc)
        assert sim_ref.untouched(filt) and sim_ref.untouched(guard) and pos == (-12345, -12345), kw
    out = np.full((16, 16), sim_ref.SENTINEL)
    pos = np.zeros(2, dtype=np.int64)
    F = np.ascontiguousarray(sim_ref.seeded_features(5, 20))
    for args in ((None, 5, 20, 5, 3.0, 0.0, 1.0, _ffi.as_f64p(out), _ffi.as_i64p(pos)),
                 (_ffi.as_f64p(F), 5, 20, 21, 3.0, 0.0, 1.0, _ffi.as_f64p(out), _ffi.as_i64p(pos)),
                 (_ffi.as_f64p(F), 0, 20, 5, 3.0, 0.0, 1.0, _ffi.as_f64p(out), _ffi.as_i64p(pos)),
                 (_ffi.as_f64p(F), 5, 20, 5, 3.0, -1.0, 1.0, _ffi.as_f64p(out), _ffi.as_i64p(pos))):
        assert gpu_lib.paa_thumbnail_f64(*args) == _ffi.ERR_ARG
    assert sim_ref.untouched(out)


# ---------------------------------------------------------------------------------------------------------
# both stages through features
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vec", [1151, 3001])
def test_thumbnail_through_features(gpu_lib, n_vec):
    M = 20
    F = sim_ref.clip_features(n_vec, seed=n_vec)
    ref = sim_ref.thumbnail_filter(O.self_similarity_matrix(F), M, 10.0, 0, 1, dtype=np.float64)
    ref_pos, margin = sim_ref.argmax_margin(ref)
    assert margin > 100 * 1e-9 * M, "precondition: the reference's arg-max margin %g is too small" % margin
    R = n_vec - M + 1
    filt = np.full((R, R), sim_ref.SENTINEL)
    pos = np.zeros(2, dtype=np.int64)
    _ffi.check(gpu_lib.paa_thumbnail_f64(_ffi.as_f64p(F), 68, n_vec, M, 10.0, 0.0, 1.0, _ffi.as_f64p(filt),
                                         _ffi.as_i64p(pos)))
    _cmp_nan(filt, ref, 1e-9 * M, "thumbnail through features, %d vectors" % n_vec)
    assert (int(pos[0]), int(pos[1])) == ref_pos
