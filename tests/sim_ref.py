"""np.longdouble restatement of the similarity / thumbnail stage (audioSegmentation.py:40-55, 1141-1165) -- the high
precision second opinion for pyaudioanalysis_amd/csrc/kernels_sim.hpp -- plus a helper that runs the two device entry
points on buffers with a chosen leading dimension, NaN padding, sentinel pre-fill and a guard band.
Test helper, not part of the package."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps          # scikit-learn's constant-feature rule is stated with the float64 epsilon
SENTINEL = -7.0e300                     # no similarity (|s| <= 1 or NaN) and no window sum (|s| <= M) equals it


# ---------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------
def row_stats(F, dtype=LD):
    """(mean, var, bound, rounding) per feature row, in `dtype`.  A row counts as constant when var <= bound =
    n eps var + (n mean eps)^2 (scikit-learn >= 0.24, written as oracle/paa_oracle.py:standardize_rows).
    `rounding` bounds what float64 evaluation can move var - bound by: every d_t = x_t - mean carries an absolute error
    of at most eps max|x| (the rounded mean and the rounded difference), which enters sum d^2 through 2 |d_t|, and the
    n-term sums add n eps of their own value."""
    X = np.asarray(F, dtype=dtype)
    n = X.shape[1]
    mean = X.sum(axis=1) / n
    d = X - mean[:, None]
    corr = d.sum(axis=1)
    var = ((d * d).sum(axis=1) - corr * corr / n) / n
    bound = n * dtype(EPS) * var + (n * mean * dtype(EPS)) ** 2
    rounding = dtype(EPS) * (2 * np.abs(X).max(axis=1) * np.abs(d).mean(axis=1) + n * var + n * bound)
    return mean, var, bound, rounding


def standardize_rows(F, dtype=LD):
    X = np.asarray(F, dtype=dtype)
    mean, var, bound, _ = row_stats(X, dtype)
    scale = np.sqrt(var)
    scale[var <= bound] = 1
    return (X - mean[:, None]) / scale[:, None]


def self_similarity(F, dtype=LD):
    """1 - squareform(pdist(Z.T, 'cosine')): cosine of the standardised columns, clipped to [-1, 1], similarity =
    1 - (1 - cos), unit diagonal (squareform's zero diagonal); zero vectors give NaN = 0/0 off the diagonal."""
    Z = standardize_rows(F, dtype)
    norms = np.sqrt((Z * Z).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (Z.T @ Z) / (norms[:, None] * norms[None, :])
    big = np.abs(cos) > 1
    cos[big] = np.copysign(dtype(1), cos[big])
    sim = 1 - (1 - cos)
    np.fill_diagonal(sim, 1)
    return sim


def window_sums(S, M, dtype=LD):
    """convolve2d(S, eye(M), 'valid') as direct window sums: out[i][j] = sum_{k < M} S[i + k][j + k].  A NaN is
    forgotten as soon as it leaves the window."""
    S = np.asarray(S, dtype=dtype)
    R = S.shape[0] - M + 1
    if R < 1:
        raise ValueError("fewer vectors (%d) than the filter length (%d)" % (S.shape[0], M))
    out = np.zeros((R, R), dtype=dtype)
    for k in range(M):
        out += S[k:k + R, k:k + R]
    return out


def mask(R, band, limit_1, limit_2):
    """True where audioSegmentation.py:1149-1160 overwrites with the minimum; band is the reference's 5.0 / short_step."""
    i = np.arange(R)
    m = (np.abs(i[:, None] - i[None, :]) < band) | (i[:, None] > i[None, :])
    m[0:int(limit_1 * R), :] = True
    m[:, 0:int(limit_1 * R)] = True
    m[int(limit_2 * R):, :] = True
    m[:, int(limit_2 * R):] = True
    return m


def thumbnail_filter(S, M, band, limit_1=0, limit_2=1, dtype=LD):
    """The masked filtered matrix: minimum taken BEFORE masking (NaN if any window holds one, as np.min), masks in the
    reference's order."""
    out = window_sums(S, M, dtype)
    R = out.shape[0]
    min_sm = np.min(out)
    i = np.arange(R)
    out[(np.abs(i[:, None] - i[None, :]) < band) | (i[:, None] > i[None, :])] = min_sm
    out[0:int(limit_1 * R), :] = min_sm
    out[:, 0:int(limit_1 * R)] = min_sm
    out[int(limit_2 * R):, :] = min_sm
    out[:, int(limit_2 * R):] = min_sm
    return out


def argmax_margin(filtered):
    """((row, column) of numpy.argmax -- first maximum in row-major order, NaN first --, decision margin = gap between
    the largest and the second-largest distinct value; inf when there is one distinct value, nan when NaN decides)."""
    pos = tuple(int(v) for v in np.unravel_index(np.argmax(filtered), filtered.shape))
    if np.isnan(filtered).any():
        return pos, float("nan")
    u = np.unique(filtered)
    return pos, (float(u[-1] - u[-2]) if u.size > 1 else float("inf"))


# ---------------------------------------------------------------------------------------------------------
# device entry points on guarded buffers
# ---------------------------------------------------------------------------------------------------------
def _filled(count):
    return np.full(int(count), SENTINEL)


def dev_self_similarity(lib, F, ld=None, guard_rows=2):
    """paa_dev_self_similarity of F [n_dims][n_vec] stored with leading dimension ld (padding columns = NaN) into a
    sentinel-filled buffer with guard_rows extra rows.  Returns (rc, S [n_vec][n_vec], guard [guard_rows * n_vec])."""
    from pyaudioanalysis_amd import _ffi
    F = np.asarray(F, dtype=np.float64)
    n_dims, n = F.shape
    ld = n if ld is None else int(ld)
    host = np.full((n_dims, ld), np.nan)
    host[:, :n] = F
    d_in = _ffi.DeviceBuffer.from_host(host)
    d_out = _ffi.DeviceBuffer.from_host(_filled((n + guard_rows) * n))
    try:
        rc = lib.paa_dev_self_similarity(d_in.ptr, n_dims, n, ld, d_out.ptr)
        _ffi.sync()
        flat = d_out.to_host(np.float64, (n + guard_rows) * n)
    finally:
        d_in.free()
        d_out.free()
    return rc, flat[:n * n].reshape(n, n), flat[n * n:]


def dev_thumbnail_filter(lib, S, M, band, limit_1, limit_2, guard_rows=2, null=None, n_vec=None):
    """paa_dev_thumbnail_filter of the matrix S [n][n] into a sentinel-filled buffer with guard_rows extra rows.
    Returns (rc, filtered [R][R], (row, column), guard).  null in ("sim", "filt", "pos") passes a null pointer for that
    argument; n_vec overrides the vector count handed to the entry point (error paths: the host must reject the call
    before any launch, the buffers stay as allocated for the true n)."""
    from pyaudioanalysis_amd import _ffi
    S = np.ascontiguousarray(S, dtype=np.float64)
    n = S.shape[0]
    R = max(n - int(M) + 1, 1)
    d_in = _ffi.DeviceBuffer.from_host(S)
    d_out = _ffi.DeviceBuffer.from_host(_filled((R + guard_rows) * R))
    pos = np.full(2, -12345, dtype=np.int64)
    try:
        rc = lib.paa_dev_thumbnail_filter(None if null == "sim" else d_in.ptr, n if n_vec is None else int(n_vec), int(M),
                                          float(band), float(limit_1), float(limit_2),
                                          None if null == "filt" else d_out.ptr,
                                          None if null == "pos" else _ffi.as_i64p(pos))
        _ffi.sync()
        flat = d_out.to_host(np.float64, (R + guard_rows) * R)
    finally:
        d_in.free()
        d_out.free()
    return rc, flat[:R * R].reshape(R, R), (int(pos[0]), int(pos[1])), flat[R * R:]


def untouched(a):
    """Every element still holds the sentinel, bit for bit."""
    a = np.asarray(a)
    return bool(np.array_equal(a.view(np.int64), np.full(a.shape, SENTINEL).view(np.int64)))


def same_bits(a, b):
    """Equal as bit patterns, except that any NaN equals any NaN (the payload of a produced NaN is not specified)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ---------------------------------------------------------------------------------------------------------
# input generators (every one is run once, and its promised properties asserted, in tests/test_sim_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------
SIM_N_VEC = (1, 2, 127, 128, 129, 255, 256, 257, 384, 385, 1151)
SIM_N_DIMS = (1, 3, 4, 5, 31, 32, 33, 36, 64, 68, 136)


def persistent_n_vec():
    """Smallest tile count whose triangle has more than 512 tiles (2 x 256 compute units, so every persistent workgroup
    takes a second tile and most a third), and a vector count that ends 71 columns into the last tile."""
    tiles = 1
    while tiles * (tiles + 1) // 2 <= 512:
        tiles += 1
    return (tiles - 1) * 128 + 71, tiles


def sim_shape_cases():
    """Pairwise-covering subset of SIM_N_VEC x SIM_N_DIMS: a cyclic Latin-square walk gives every n_vec three different
    n_dims and every n_dims three different n_vec (33 of the 121 pairs; each value of either axis meets each class of the
    other -- multiple of 4 or not, below / at / above the 32-row chunk, tile-aligned or not).  Plus the persistent size."""
    cases = []
    for a, n in enumerate(SIM_N_VEC):
        for s in (0, 4, 7):
            cases.append((n, SIM_N_DIMS[(a + s) % len(SIM_N_DIMS)]))
    big, _ = persistent_n_vec()
    cases += [(big, 68), (big, 33)]
    return cases


def seeded_features(n_dims, n_vec, seed=0):
    rng = np.random.default_rng(1000003 * n_dims + 7 * n_vec + seed)
    return rng.standard_normal((n_dims, n_vec)) * rng.uniform(0.1, 50.0, (n_dims, 1)) + rng.uniform(-5, 5, (n_dims, 1))


def exact_zero_features(n_dims, half, zero_cols, seed=0):
    """Integer-valued [V, -V] (row means exactly 0, every sum exact) with exact zero vectors at zero_cols (mirrored into
    the second half so that the means stay 0).  Returns (F [n_dims][2 half], sorted zero columns)."""
    rng = np.random.default_rng(seed)
    V = rng.integers(-9, 10, (n_dims, half)).astype(np.float64)
    V[:, np.all(V == 0, axis=0)] = 1.0
    zc = sorted(set(int(c) % half for c in zero_cols))
    V[:, zc] = 0.0
    F = np.concatenate([V, -V], axis=1)
    return F, sorted(zc + [c + half for c in zc])


def duplicate_features(n_dims, quarter, seed=0):
    """Integer-valued [A, -A, A, -A] (row means exactly 0, one scale per row): column i + 2 quarter standardises to the
    same vector as column i and column i + quarter to its negation; column 1 repeats column 0.
    Returns (F [n_dims][4 quarter], [(i, j, +1 or -1)])."""
    rng = np.random.default_rng(seed)
    q = int(quarter)
    A = rng.integers(-64, 65, (n_dims, q)).astype(np.float64)
    A[0, :] += 100.0                                  # no zero column
    if q > 1:
        A[:, 1] = A[:, 0]
    F = np.concatenate([A, -A, A, -A], axis=1)
    pairs = [(0, q, -1), (0, 2 * q, 1), (0, 3 * q, -1), (q - 1, 2 * q - 1, -1), (q - 1, 3 * q - 1, 1),
             (q - 1, 4 * q - 1, -1)]
    if q > 1:
        pairs += [(0, 1, 1), (1, q, -1)]
    return np.ascontiguousarray(F), pairs


CONDITIONING_CASES = ("offset_1e3", "offset_1e6", "offset_1e9", "near_constant")


def conditioning_features(case):
    """20 x 300 Gaussian rows with a large offset (mean / sigma of 1e3, 1e6, 1e9), or -- near_constant -- unit-scale rows
    of which row 5 is 1 + k ulp with a spread 1000 x the constant-row threshold n |mean| eps (not constant) and row 9 the
    same with a spread a tenth of the threshold (constant: scale 1)."""
    rng = np.random.default_rng(20 + CONDITIONING_CASES.index(case))
    F = rng.standard_normal((20, 300))
    if case == "near_constant":
        ulp = EPS
        thr = 300 * EPS                                    # sigma at which var = (n mean eps)^2 for mean = 1
        F[5] = 1.0 + np.round(rng.standard_normal(300) * (1000 * thr / ulp)) * ulp
        F[9] = 1.0 + np.round(rng.standard_normal(300) * (0.1 * thr / ulp)) * ulp
    else:
        F = F + float(case.split("_")[1])
    return F


# thumbnail stage: symmetric matrices of multiples of 1/8 in [-1, 1] -> every window sum and sliding update is exact
def dyadic_matrix(n, seed, levels=8):
    rng = np.random.default_rng(seed)
    A = rng.integers(-levels, levels + 1, (n, n)).astype(np.float64) / levels
    S = np.triu(A) + np.triu(A, 1).T
    return np.ascontiguousarray(S)


def tied_matrix(n, period=24):
    """Periodic symmetric matrix over {0, 1/2, 1}: S[i][j] depends on (i mod period, j mod period) symmetrically, so
    every window sum repeats along both axes and the maximum occurs once per period pair."""
    i = np.arange(n) % period
    base = ((i[:, None] * 7 + i[None, :] * 7 + (i[:, None] * i[None, :]) % 5) % 3).astype(np.float64) / 2.0
    return np.ascontiguousarray(base)


def tie_spread(filtered):
    """(count of cells holding the maximum, distinct thumb_diag x blocks, y blocks, waves within a block) of the unmasked
    maxima: thread = diagonal offset d = j - i (256 per x block, 64 per wave), 32 rows per y block."""
    mx = np.max(filtered)
    ii, jj = np.nonzero(filtered == mx)
    up = jj >= ii
    ii, jj = ii[up], jj[up]
    d = jj - ii
    return int(ii.size), len(set(d // 256)), len(set(ii // 32)), len(set((d % 256) // 64))


def clip_features(n_vec, seed):
    """Well-conditioned 68-row clip for the two stages through features: a slow random walk (similarities spread over
    [-1, 1]) with two planted repeats of one passage, so that the filtered maximum stands clear of the runner-up."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((68, n_vec)).cumsum(axis=1) * 0.05 + rng.standard_normal((68, n_vec))
    L = 60
    a, b = n_vec // 5, (3 * n_vec) // 5
    passage = 6.0 * rng.standard_normal((68, L))
    F[:, a:a + L] = passage + 0.05 * rng.standard_normal((68, L))
    F[:, b:b + L] = passage + 0.05 * rng.standard_normal((68, L))
    return np.ascontiguousarray(F)


# thumbnail stage alone: (n, M) with R = n - M + 1 in {1, 2, 31, 32, 33, 255, 256, 257, 1023, 1025, 2049} (more than one
# thumb_fill x block above 1024, nine thumb_diag x blocks at 2049) and M in {1, 2, 31, 32, 33, 64, n}
THUMB_SIZES = ((40, 40), (3, 2), (31, 1), (62, 31), (64, 32), (287, 33), (319, 64), (258, 2), (1023, 1), (1056, 32),
               (2112, 64), (2079, 31))
THUMB_BANDS = ("0", "0.5", "1", "10", "R", "R+5")
THUMB_LIMITS = ((0, 1), (0.1, 0.9), (0.5, 0.5), (0.9, 0.1), (0, 0), (0, 1.5))
# limit * R just below / at / just above an integer in float64: int() truncation must agree with Python's
THUMB_TRUNC = ((10, 0.3, 0.7), (100, 0.3, 0.7), (100, 0.29, 0.57), (10, 0.7, 0.9), (100, 0.07, 0.58))
THUMB_NAN_M = (1, 7, 31, 40)


def band_value(name, R):
    return {"0": 0.0, "0.5": 0.5, "1": 1.0, "10": 10.0, "R": float(R), "R+5": float(R + 5)}[name]


def degenerate_matrices(n, band):
    """name -> matrix: 'constant' (every window sum equal), 'max_is_min' (values above the minimum only closer to the
    diagonal than the band, so the unmasked maximum is the global minimum)."""
    const = np.full((n, n), 0.5)
    i = np.arange(n)
    near = np.abs(i[:, None] - i[None, :]) < max(int(band) - 1, 1)
    return {"constant": const, "max_is_min": np.where(near, 0.75, 0.25)}


def nan_matrices(n, seed):
    """name -> dyadic matrix with NaN planted symmetrically: one cell whose row index is a thumb_diag run start (64), mid
    run (80) or run end (95), one whole row and column, everything."""
    out = {}
    for name, a in (("run_start", 64), ("mid_run", 80), ("run_end", 95)):
        S = dyadic_matrix(n, seed)
        S[a, a + 50] = S[a + 50, a] = np.nan
        out[name] = S
    S = dyadic_matrix(n, seed)
    S[70, :] = np.nan
    S[:, 70] = np.nan
    out["row_and_column"] = S
    out["all"] = np.full((n, n), np.nan)
    return out
