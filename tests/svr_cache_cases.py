"""The inputs, the exact restatement and the derived bounds of the resident-kernel-matrix tests of the SVR solver, shared by
tests/test_svr_cache_cpu.py (which checks the restatement, the bounds and the packing rule without a device) and
tests/test_svr_cache_gpu.py (which runs svr_standardise_kernel, svr_gram_kernel and svr_smo_cached_kernel).  Test helper, not part
of the package.

The Gram kernel's value for two standardised rows z, z' of n_dims dims is a chain: lane l of 8 runs acc = fma(a, b, acc) over the
dims l, l + 8, ... (M = ceil(n_dims / 8) steps), three additions fold the 8 partial sums, and the RBF kernel takes exp(-gamma acc).
With u = 2^-53, every fma and every addition rounds once, so a term passes through at most M + 3 roundings:

    linear   |K - sum z z'|  <=  (M + 3) u sum |z z'|                                   (the bound the issue states)
    RBF      a term is fl(z - z')^2: one more rounding, squared, (1 + u)^2 <= 1 + 2 u + u^2, so the chain's exponent acc lies
             within (M + 3 + 3) u E of E = sum (z - z')^2 (every term is >= 0, so sum |term| = E; the 3 covers 2 u + u^2 and its
             products with the (M + 3) u above for any M <= 32).  The product gamma acc rounds once more and exp is held to one
             ulp, so with x = gamma E and dx = gamma (M + 6) u E + u gamma E (1 + (M + 6) u):
             |K - exp(-x)|  <=  exp(-x) expm1(dx) + ulp(exp(-x))

The exact sums come from integers: Z 2^k is a matrix of integers for a k read from the data; split into limbs of 21 bits, every
limb product summed over <= 256 dims stays below 2^50 and is exact in a float64 matmul, and Python integers put the limbs
together.  The RBF reference exp(-gamma E) is formed in double from the correctly rounded E (one rounding), the rounded product
(one more) and the C library's exp (held to one ulp): 2 u x exp(-x) + ulp, added to the bound as the reference's own error."""
import functools
import math

import numpy as np

U = 2.0**-53
LIMB = 21
GRAM_ROWS = (1, 2, 17, 33, 257)
GRAM_DIMS = (1, 9, 136, 256)
FINAL_FITS = (("rbf", 0.01), ("rbf", 0.1), ("rbf", 1.0), ("linear", 0.01))     # above C = 0.01 the linear dual's path is decided by roundings
MAX_ROWS = 8192


def chain_steps(n_dims):
    return (n_dims + 7) // 8


# ---------------------------------------------------------------------------------------------------------------------
# the exact Gram matrix in integers
# ---------------------------------------------------------------------------------------------------------------------
def _limbs(Z):
    """(signed limb matrices of Z 2^k, least first; k): Z 2^k is integer-valued."""
    nz = Z != 0
    if not nz.any():
        return [np.zeros_like(Z)], 0
    _, e = np.frexp(Z[nz])
    k = max(53 - int(e.min()), 0)                       # |z| = m 2^e with m 2^53 an integer
    a = np.ldexp(np.abs(Z), k)
    assert np.all(a == np.floor(a)) and a.max() < 2.0**1000
    out = []
    while a.max() > 0:
        low = np.fmod(a, 2.0**LIMB)
        out.append(np.sign(Z) * low)
        a = (a - low) / 2.0**LIMB
    return out, k


def _int_product(A, B):
    """The integer matrix (sum_p A_p 2^(21 p)) (sum_q B_q 2^(21 q))^T of limb lists, as an object array of Python integers."""
    assert A[0].shape[1] <= 256
    total = np.zeros((A[0].shape[0], B[0].shape[0]), dtype=object)
    for p, a in enumerate(A):
        for q, b in enumerate(B):
            part = a @ b.T                              # |entries| < 2^21 2^21 256 = 2^50: exact
            total = total + part.astype(np.int64).astype(object) * (1 << (LIMB * (p + q)))
    return total


def exact_gram(Z):
    """(G, A, k): G = (Z 2^k)(Z 2^k)^T and A = |Z 2^k| |Z 2^k|^T as Python integers, exact."""
    limbs, k = _limbs(np.asarray(Z, dtype=np.float64))
    return _int_product(limbs, limbs), _int_product([np.abs(m) for m in limbs], [np.abs(m) for m in limbs]), k


def _to_int(K, shift):
    """K 2^shift as Python integers; K must be a multiple of 2^-shift (a value of the chain is: see check_linear)."""
    scaled = np.ldexp(np.asarray(K, dtype=np.float64), shift)
    assert np.all(scaled == np.floor(scaled))
    return np.vectorize(int, otypes=[object])(scaled)


def linear_violations(K, Z, roundings=None):
    """(the number of values of K outside `roundings` u sum |z z'| of the exact sum -- None: the chain's M + 3; the errors and
    the sums of |z z'|, both times 2^2k, as integers).  Every product z z' is a multiple of 2^-2k and
    rounding a multiple of 2^-2k keeps one, so a chain value times 2^2k is an integer: the comparison is exact."""
    G, A, k = exact_gram(Z)
    err = np.abs(_to_int(K, 2 * k) - G)
    roundings = chain_steps(Z.shape[1]) + 3 if roundings is None else roundings
    return int(np.count_nonzero(err * (1 << 53) > roundings * A)), err, A


def rbf_reference(Z, gamma):
    """(exp(-gamma E) in double, x = gamma E in double, E exact over 2^2k as integers, k)."""
    G, _, k = exact_gram(Z)
    d = np.diagonal(G)
    E_int = d[:, None] + d[None, :] - 2 * G             # sum (z - z')^2 2^2k, exact
    E = np.vectorize(lambda v: v / (1 << (2 * k)), otypes=[np.float64])(E_int)         # int / int: correctly rounded
    x = gamma * E
    return np.vectorize(math.exp, otypes=[np.float64])(-x), x, E_int, k


def rbf_bound(x, ref, n_dims, roundings=None):
    """The bound of the module docstring on |K - ref|, the reference's own error included (roundings: M + 6 of the chain)."""
    c = (chain_steps(n_dims) + 6 if roundings is None else roundings) * U
    dx = x * c + U * x * (1 + c)
    return ref * np.expm1(dx) + np.spacing(ref) + (2 * U * x * ref + np.spacing(ref))


def rbf_violations(K, Z, gamma, roundings=None):
    ref, x, _, _ = rbf_reference(Z, gamma)
    return int(np.count_nonzero(np.abs(K - ref) > rbf_bound(x, ref, Z.shape[1], roundings)))


def chain_gram(Z, kernel, gamma):
    """The Gram kernel's chain in NumPy, term by term in its order -- with TWO roundings per step where the device's fma has one,
    so it stays within the bound with M + 3 replaced by 2 M + 3, not bit-equal: what the CPU test holds against the bounds."""
    n, d = Z.shape
    M = chain_steps(d)
    P = np.zeros((n, 8 * M))
    P[:, :d] = Z
    acc = np.zeros((n, n, 8))
    for i in range(M):
        a, b = P[:, None, 8 * i:8 * i + 8], P[None, :, 8 * i:8 * i + 8]
        acc = acc + ((a - b) * (a - b) if kernel == "rbf" else a * b)
    for o in (1, 2, 4):
        acc = acc + acc[:, :, np.arange(8) ^ o]
    return np.exp(-gamma * acc[:, :, 0]) if kernel == "rbf" else acc[:, :, 0]


@functools.lru_cache(maxsize=None)
def gram_inputs(n_dims):
    """(X, tasks (rows, mean, scale, gamma)) of the Gram kernel's own test at n_dims: one task per row count of GRAM_ROWS, each
    standardised with the statistics of its own rows (of all samples for fewer than 4 rows)."""
    rng = np.random.default_rng(900 + n_dims)
    X = rng.standard_normal((300, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    tasks = []
    for n in GRAM_ROWS:
        rows = rng.permutation(300)[:n]
        src = X[rows] if n > 3 else X
        tasks.append((rows, src.mean(axis=0), src.std(axis=0), 0.7 / n_dims))
    return X, tasks


# ---------------------------------------------------------------------------------------------------------------------
# the packing rule, counted by hand
# ---------------------------------------------------------------------------------------------------------------------
def matrix_bytes(n):
    return 8 * n * n


# (row counts, budget, the chunk of every task: -1 is "not cached")
PACKING_BY_HAND = (
    ((1, 1, 1), 8, (0, 1, 2)),                          # 8 bytes each: one task per chunk
    ((1, 1, 1), 16, (0, 0, 1)),
    ((1, 1, 1), 24, (0, 0, 0)),
    ((2, 1, 2), 8, (-1, 0, -1)),                        # 32 > 8: only the one-row task is cached
    ((2, 1, 2), 39, (0, 1, 2)),                         # 32 | 32 + 8 = 40 > 39 | 8 + 32 > 39
    ((2, 1, 2), 40, (0, 0, 1)),                         # 32 + 8 = 40 fits exactly | 40 + 32 > 40
    ((3, 3, 3, 3), 144, (0, 0, 1, 1)),                  # 72 each: two per chunk exactly
    ((3, 3, 3, 3), 143, (0, 1, 2, 3)),
    ((10, 1, 10, 1), 800, (0, 1, 2, 3)),                # 800 | 800 + 8 > 800 | 8 + 800 > 800 | 800 + 8 > 800
    ((10, 1, 10, 1), 808, (0, 0, 1, 1)),
    ((3, 100, 3), 144, (0, -1, 0)),                     # a task that is not cached does not close the open chunk
    ((1025, 3, 1025), matrix_bytes(1025), (0, 1, 2)),   # 8 405 000 | + 72 > | 72 + 8 405 000 >
    ((1025, 3, 1025), matrix_bytes(1025) - 1, (-1, 0, -1)),
    ((1025, 3, 1025), matrix_bytes(1025) + 72, (0, 0, 1)),
    ((8192,) * 9, 5 << 30, (0,) * 9),                   # 9 x 512 MiB = 4.5 GiB under 5 GiB
    ((8192,) * 9, 4 << 30, (0,) * 8 + (1,)),
)


def expected_cached(rows, cache_bytes):
    """The `cached` flags the rule implies: a task is cached exactly when its own matrix fits the budget."""
    return np.array([matrix_bytes(int(n)) <= cache_bytes for n in rows])


# ---------------------------------------------------------------------------------------------------------------------
# the final fit on the goldens' 240 x 12 problem
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def final_fit_case(kernel, C):
    """(Z, y, scikit-learn's fitted SVR, its predictions of the training rows, the restatement's, tol): Z the goldens' samples
    standardised as feature_extraction_train_regression standardises them; tol is the goldens' rule, max(4 x the distance
    between the restatement and scikit-learn, 1e-9), the distance relative to max |prediction|."""
    import sklearn.svm

    import svr_fit_ref
    import train_ref
    g = train_ref.load_golden("svr_fit_" + kernel)
    X, y = np.asarray(g["X"], dtype=np.float64), np.asarray(g["y"], dtype=np.float64)
    assert X.shape == (240, 12)
    Z = (X - X.mean(axis=0)) / X.std(axis=0)
    sk = sklearn.svm.SVR(C=C, kernel=kernel).fit(Z, y)
    sk_pred = sk.predict(Z)
    rows = np.arange(240)
    ref_pred = svr_fit_ref.fit_job(Z, y, (rows, rows, np.zeros(12), np.ones(12), C), kernel)[0]
    distance = np.max(np.abs(ref_pred - sk_pred)) / np.max(np.abs(sk_pred))
    return Z, y, sk, sk_pred, ref_pred, max(4 * distance, 1e-9)
