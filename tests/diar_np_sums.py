"""The three sums that k-means++ seeding forms with NumPy in the loop of single calls (audioSegmentation._diar_seed), restated
element by element: the device seeding of the batch (kernels_diarbatch.hpp, seed_kernel) walks them in exactly this order, so
that clip i of a batch carries the bits of its own single call.  tests/test_diar_batch_cpu.py pins every function here against
NumPy itself; a NumPy that sums differently shows up there and not as a GPU mismatch.

  * pairwise: NumPy's pairwise summation of at most 8192 contiguous elements: serial below 8 elements; up to 128 elements eight
    strided accumulators combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and the tail added serially; above 128
    the run is split at n / 2 rounded down to a multiple of 8.
  * sum_1d: closest.sum() on a contiguous vector, and sum_rows: new.sum(axis=1) on a C-contiguous [trials][n] array -- the
    pairwise sum of every chunk of 8192 elements (NumPy's reduction buffer), the chunk results added serially in order.  Both
    follow this one rule (measured against NumPy 2.2.6 on fresh vectors and on row views of a 2-D array, which is what
    `closest = new[best]` is): a vector of more than 8192 elements is NOT summed pairwise as a whole.
  * cumsum: np.cumsum -- serial."""
import numpy as np

BLOCK = 128
CHUNK = 8192


def _leaf(a):
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    r = [np.float64(v) for v in a[:8]]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + a[i]
        i += 1
    return res


def pairwise(a):
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    if n <= BLOCK:
        return _leaf(a)
    half = n // 2
    half -= half % 8
    return pairwise(a[:half]) + pairwise(a[half:])


def sum_1d(a):
    a = np.asarray(a, dtype=np.float64)
    res = np.float64(0.0)
    for c0 in range(0, len(a), CHUNK):
        res = res + pairwise(a[c0:c0 + CHUNK])
    return res


def sum_rows(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([sum_1d(row) for row in a], dtype=np.float64).reshape(a.shape[0])


def cumsum(a):
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(len(a))
    c = np.float64(0.0)
    for i, v in enumerate(a):
        c = c + v
        out[i] = c
    return out


def seed_draws(rs, n, ks, given=()):
    """The numbers one clip's sweep takes from `rs`, in order: per k without given centres randint(n), then (k - 1) times
    uniform(size = 2 + int(ln k)).  Returns {k: (first, u [k - 1][trials])}."""
    out = {}
    for k in ks:
        if k in given:
            continue
        trials = 2 + int(np.log(k))
        first = int(rs.randint(n))
        out[k] = (first, np.array([rs.uniform(size=trials) for _ in range(1, k)]).reshape(k - 1, trials))
    return out
