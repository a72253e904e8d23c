"""The inputs of the SMO solver's edge tests, shared by tests/test_smo_edges_ref_cpu.py (which asserts, on the restatement of
tests/smo_ref.py alone, the conditions that make each input meaningful) and tests/test_smo_edges_gpu.py (which runs them through
smo_kernel / svc_pairs_kernel).  Plain NumPy; imports nothing from the package.

A solver task is what audioTrainTest.smo_solve takes: (rows, signs, mean, scale, C, gamma); a vote job what
svm_split_fit_predict takes: (train_idx, test_idx, mean, scale, C)."""
import collections
import functools

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# (a) the trajectory set: tasks whose every selection is decided by a margin far above rounding, so that the path of a
#     correct solver is the restatement's, step by step
# ---------------------------------------------------------------------------------------------------------------------
N_TRAJECTORY_SAMPLES = 160
N_INTEGER_SAMPLES = 8                   # appended to the matrix: small integers, read with mean 0 / scale 1 by the TAU tasks

Trajectory = collections.namedtuple("Trajectory", "name n_dims kernel eps task tau")
# (n_dims, kernel, rows, C, eps, seed, gamma (None: 1 / n_dims)): fixed seeds, found by a search over the restatement for
# tasks that meet the conditions of test_smo_edges_ref_cpu.py
TRAJECTORY_SPECS = (
    (1, "linear", 70, 1.0, 1e-3, 24, None),
    (1, "rbf", 5, 1.0, 1e-3, 29, None),
    (1, "rbf", 5, 0.05, 1e-3, 10, None),
    (1, "rbf", 5, 0.05, 1e-3, 10, 0.37),               # the task above under another gamma, in the same batch
    (1, "rbf", 33, 1.0, 1e-2, 30, None),
    (9, "linear", 2, 1.0, 1e-3, 0, None),
    (9, "linear", 70, 0.05, 1e-3, 11, None),
    (9, "linear", 16, 0.05, 1e-3, 5, None),
    (9, "linear", 12, 1.0, 1e-2, 30, None),
    (9, "linear", 33, 20.0, 1e-1, 56, None),
    (9, "rbf", 70, 0.05, 1e-3, 44, None),
    (9, "rbf", 33, 1.0, 1e-2, 32, None),
    (9, "rbf", 33, 1.0, 1e-2, 32, 0.37 / 3.0),         # likewise
    (9, "rbf", 47, 20.0, 1e-2, 12, None),
    (256, "linear", 12, 1.0, 1e-1, 1, None),
    (256, "rbf", 70, 0.05, 1e-3, 31, None),
    (256, "rbf", 33, 1.0, 1e-2, 43, None),
)


def trajectory_matrix(n_dims):
    """(X [160 + 8][n_dims], y [160 + 8]): two overlapping Gaussian classes in alternation, then the integer rows
    (0, ..), (1, 0, ..), (2, 0, ..), ... with signs + - + - ...: row 160 + k has k in its first column and zeros elsewhere."""
    rng = np.random.default_rng(700 + n_dims)
    n = N_TRAJECTORY_SAMPLES
    y = np.where(np.arange(n + N_INTEGER_SAMPLES) % 2 == 0, 1.0, -1.0)
    X = rng.standard_normal((n, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    X += 1.5 * y[:n, None] / np.sqrt(n_dims)
    ints = np.zeros((N_INTEGER_SAMPLES, n_dims))
    ints[:, 0] = np.arange(N_INTEGER_SAMPLES)
    return np.vstack([X, ints]), y


def _own_stats(X, rows):
    mean, scale = X[rows].mean(axis=0), X[rows].std(axis=0)
    return mean, np.where(scale > 0, scale, 1.0)


@functools.lru_cache(maxsize=None)
def trajectory_tasks():
    """[Trajectory]: the random tasks of TRAJECTORY_SPECS (each standardised with the statistics of its own rows), the pairs
    that differ in gamma alone, and the TAU tasks: integer rows under mean 0 / scale 1 and the linear kernel, among them two
    rows with the SAME sample index and opposite signs, so that eta of that pair is exactly 0."""
    out = []
    for n_dims, kernel, n, C, eps, seed, gamma in TRAJECTORY_SPECS:
        X, y = trajectory_matrix(n_dims)
        rows = np.random.default_rng(seed * 1000 + n).permutation(N_TRAJECTORY_SAMPLES)[:n]
        mean, scale = _own_stats(X, rows)
        name = "d%d_%s_n%d_C%g_s%d%s" % (n_dims, kernel, n, C, seed, "" if gamma is None else "_g%g" % gamma)
        out.append(Trajectory(name, n_dims, kernel, eps, (rows, y[rows], mean, scale, C, gamma), False))
    # integer samples 160 + k = (k, 0, ..).  tau4: i of step 1 is the last positive row (sample 2) and its twin the last row;
    # the pair ends at C on both sides and the other two rows then separate 1 from 3.  tau6: the twins (sample 7) meet at step 3
    for n_dims, name, samples, signs in ((1, "tau4", (1, 3, 2, 2), (1, -1, 1, -1)), (9, "tau6", (7, 2, 4, 6, 7, 3), (1, 1, 1, -1, -1, -1)),
                                         (256, "tau4", (1, 3, 2, 2), (1, -1, 1, -1))):
        task = (N_TRAJECTORY_SAMPLES + np.array(samples), np.array(signs, dtype=np.float64), np.zeros(n_dims), np.ones(n_dims), 1.0, None)
        out.append(Trajectory("d%d_%s" % (n_dims, name), n_dims, "linear", 1e-3, task, True))
    return out


def trajectory_batches():
    """{(n_dims, kernel, eps): [Trajectory]}: what one smo_solve call can take together."""
    out = collections.OrderedDict()
    for t in trajectory_tasks():
        out.setdefault((t.n_dims, t.kernel, t.eps), []).append(t)
    return out


def standardised(X, task):
    """The rows of a task as the kernels read them."""
    return (X[task[0]] - task[2]) / task[3]


# ---------------------------------------------------------------------------------------------------------------------
# (b) exact ties at iteration 0
# ---------------------------------------------------------------------------------------------------------------------
TIE_ROWS = (2, 9, 33, 65, 257, 1025)
EDGE_POSITIONS = (0, 7, 8, 31, 32, 33, 63, 64, 255, 256)       # group, wave and stride edges: row t is in group t % 32
TIE_DIMS, TIE_C = 3, 1.0
_N_OTHER = 40

TieLayout = collections.namedtuple("TieLayout", "name task i j n_positive n_tied_j")


def tie_matrix():
    """Integer samples in 3 dims (every kernel value, eta and gradient of step 1 is exact in any order of summation):
    0: the positive row that has to be chosen, the origin; 1: the nearest negative, (1, 1, 1), eta = 3;
    2 .. 41: other positives (-(k + 1), 1, 0); 42 .. 81: farther negatives (2 + k, 1, 1), eta >= 6."""
    k = np.arange(_N_OTHER)
    other = np.stack([-(k + 1.0), np.ones(_N_OTHER), np.zeros(_N_OTHER)], axis=1)
    far = np.stack([2.0 + k, np.ones(_N_OTHER), np.ones(_N_OTHER)], axis=1)
    return np.vstack([[[0.0, 0, 0], [1.0, 1, 1]], other, far])


def _tie_positions(n):
    return [p for p in sorted(set(EDGE_POSITIONS + (n - 1,))) if p < n]


@functools.lru_cache(maxsize=None)
def tie_layouts():
    """[TieLayout].  At alpha = 0, G = -1 every positive row has v = 1 and ties for i; the positives are the position p and
    the positions t < p with t % 3 == 1 (distinct samples: another i gives other values).  The negatives:
    kind "one": all the nearest sample -- every negative ties for j;
    kind "scattered": the nearest sample at a position q taken from the same edges, and at the negative positions t < q
    with t % 5 == 0 (at least one); every other negative, before and after q, is a farther sample."""
    zeros, ones = np.zeros(TIE_DIMS), np.ones(TIE_DIMS)
    out = []
    for n in TIE_ROWS:
        positions = _tie_positions(n)
        for at, p in enumerate(positions):
            positive = np.zeros(n, dtype=bool)
            positive[p] = True
            positive[[t for t in range(p) if t % 3 == 1]] = True
            negatives = np.flatnonzero(~positive)
            for kind in ("one", "scattered"):
                rows = np.where(positive, 2 + np.arange(n) % _N_OTHER, 1)
                rows[p] = 0
                if kind == "one":
                    j, n_tied = int(negatives[-1]), len(negatives)
                else:
                    cand = [q for q in sorted(set(EDGE_POSITIONS + (n - 2,)))
                            if q < negatives[-1] and not positive[q] and any(t % 5 == 0 for t in negatives[negatives < q])]
                    if n < 9 or not cand:
                        continue
                    j = cand[(at + 1) % len(cand)]
                    near = np.array([t for t in negatives if t == j or (t < j and t % 5 == 0)])
                    far = np.setdiff1d(negatives, near)
                    rows[far] = 2 + _N_OTHER + far % _N_OTHER
                    n_tied = len(near)
                task = (rows, np.where(positive, 1.0, -1.0), zeros, ones, TIE_C, None)
                out.append(TieLayout("n%d_p%d_%s_j%d" % (n, p, kind, j), task, p, j, int(np.count_nonzero(positive)), n_tied))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (c) degenerate tasks: nothing to optimise
# ---------------------------------------------------------------------------------------------------------------------
def degenerate_tasks(n_dims):
    """[(name, task)] over trajectory_matrix(n_dims): one row of either sign, five and two rows of one sign."""
    X, y = trajectory_matrix(n_dims)
    plus, minus = np.flatnonzero(y[:N_TRAJECTORY_SAMPLES] > 0), np.flatnonzero(y[:N_TRAJECTORY_SAMPLES] < 0)
    out = []
    for name, rows in (("one_plus", plus[3:4]), ("one_minus", minus[4:5]), ("five_plus", plus[5:10]), ("five_minus", minus[2:7]),
                       ("two_plus", plus[[1, 20]]), ("two_minus", minus[[0, 33]])):
        mean, scale = _own_stats(X, rows) if len(rows) > 1 else (np.zeros(n_dims), np.ones(n_dims))
        out.append((name, (rows, y[rows], mean, scale, 1.0, 0.3)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (d) - (f) vote jobs
# ---------------------------------------------------------------------------------------------------------------------
VoteCall = collections.namedtuple("VoteCall", "name X labels jobs kernel gamma tied")
TEST_ROWS = (1, 31, 32, 33, 97)


def class_value(c):
    """Class values that are no positions: 5, 8, 11, ..."""
    return 3 * c + 5


def _gaussian_classes(rng, k, n_dims, per_class, spread, n_extra, extra_spread=None, extra_shift=None):
    """(X, labels, n_train, centres): per_class[c] training rows around centre c, then n_extra further rows, around the
    centres in turn or (extra_shift given) around the centroid of the centres moved by extra_shift."""
    centres = rng.normal(0, 3.0, (k, n_dims))
    extra_centre = None if extra_shift is None else centres.mean(axis=0) + extra_shift
    X, lab = [], []
    for c in range(k):
        X.append(centres[c] + spread * rng.standard_normal((per_class[c], n_dims)))
        lab += [class_value(c)] * per_class[c]
    n_train = len(lab)
    for e in range(n_extra):
        c = e % k
        at = centres[c] if extra_centre is None else extra_centre
        X.append(at + (spread if extra_spread is None else extra_spread) * rng.standard_normal((1, n_dims)))
        lab.append(class_value(c))
    return np.vstack(X), np.array(lab), n_train, centres


def _test_list(rng, n_test, train, n_train, n_total):
    """n_test indices: further rows, some training rows and repeats."""
    extra = rng.integers(n_train, n_total, n_test)
    some_train = rng.choice(train, n_test)
    te = np.where(rng.random(n_test) < 0.25, some_train, extra)
    if n_test > 2:
        te[-1] = te[0]
    return te


# (k, n_dims, kernel, gamma, test-list lengths, seed); the k = 3 and k = 4 calls draw their test rows near the centroid of
# the centres (tied votes)
VOTE_SPECS = (
    (2, 2, "linear", None, TEST_ROWS, 11),
    (3, 2, "linear", None, (97, 33), 109),
    (4, 3, "rbf", None, (97, 32), 117),
    (8, 5, "rbf", 0.4, (31,), 14),
    (9, 9, "linear", None, (1, 97), 15),
    (16, 4, "rbf", None, (32,), 16),
    (17, 7, "linear", None, (33,), 17),
    (64, 6, "rbf", 0.05, (97,), 18),
)


@functools.lru_cache(maxsize=None)
def vote_calls():
    """[VoteCall]: one per entry of VOTE_SPECS (every job trains on all training rows, with their mean / deviation), then
    "mixed": a k = 2 job, a job with no test rows and a k = 9 job in one call."""
    out = []
    for k, n_dims, kernel, gamma, lengths, seed in VOTE_SPECS:
        rng = np.random.default_rng(seed)
        per_class = rng.integers(3, 7, k) if k >= 16 else rng.integers(7, 12, k)
        tied = k in (3, 4)
        if tied:
            X, lab, n_train, _ = _gaussian_classes(rng, k, n_dims, per_class, TIED_TRAIN_SPREAD[k], 130, TIED_SPREAD[k], TIED_SHIFT[k])
        else:
            X, lab, n_train, _ = _gaussian_classes(rng, k, n_dims, per_class, 1.0, 130)
        train = rng.permutation(n_train)
        mean, scale = X[train].mean(axis=0), X[train].std(axis=0)
        jobs = [(train, _test_list(rng, n, train, n_train, X.shape[0]), mean, scale, C) for n, C in zip(lengths, (1.0, 1.0, 0.3, 5.0, 20.0) if tied else (1.0, 5.0, 0.3, 1.0, 20.0))]
        out.append(VoteCall("k%d" % k, X, lab, jobs, kernel, gamma, tied))
    rng = np.random.default_rng(19)
    X, lab, n_train, _ = _gaussian_classes(rng, 9, 4, rng.integers(5, 9, 9), 1.0, 60)
    all_rows = rng.permutation(n_train)
    two = all_rows[(lab[all_rows] == class_value(2)) | (lab[all_rows] == class_value(7))]
    jobs = []
    for train, n_test in ((two, 33), (all_rows[:40], 0), (all_rows, 31)):
        te = _test_list(rng, n_test, train, n_train, X.shape[0]) if n_test else np.zeros(0, dtype=np.int64)
        jobs.append((train, te, X[train].mean(axis=0), X[train].std(axis=0), 2.0))
    out.append(VoteCall("mixed", X, lab, jobs, "rbf", 0.2, False))
    return out


# where the test rows of the tied calls are drawn: a point and a spread at which a good part of them falls into the region
# where the pairwise votes run in a circle (found on the restatement; test_smo_edges_ref_cpu.py asserts what they must give)
TIED_SPREAD = {3: 0.3, 4: 0.3}
TIED_SHIFT = {3: 0.0, 4: 0.0}
TIED_TRAIN_SPREAD = {3: 3.0, 4: 3.0}        # classes that overlap: the pairwise boundaries do not meet in a point

TILE_ROWS = (15, 16, 17, 32, 33)
TILE_C = 1e-4


@functools.lru_cache(maxsize=None)
def tile_calls():
    """[VoteCall], two classes, the single pair task of 15, 16, 17, 32 and 33 rows (kv::kTile is 16), the first class the
    larger where the count is odd, C = 1e-4: no row can leave the bound, so every row of the second class -- the last tile
    with them -- is a support vector."""
    out = []
    for n in TILE_ROWS:
        rng = np.random.default_rng(300 + n)
        n_b = n // 2
        X, lab, n_train, _ = _gaussian_classes(rng, 2, 5, [n - n_b, n_b], 1.0, 40)
        train = rng.permutation(n_train)
        job = (train, _test_list(rng, 33, train, n_train, X.shape[0]), X[train].mean(axis=0), X[train].std(axis=0), TILE_C)
        out.append(VoteCall("tile%d" % n, X, lab, [job], "rbf" if n % 2 else "linear", None, False))
    return out


def zero_calls():
    """[VoteCall]: X = [[+1], [-1], [0]] padded with zero columns, trained on rows 0, 1 (labels 0, 1), tested on row 2, mean 0,
    scale 1, linear, C = 1: alpha = (0.5, 0.5), rho = 0 and a decision value of exactly 0."""
    out = []
    for n_dims in (1, 9):
        X = np.zeros((3, n_dims))
        X[0, 0], X[1, 0] = 1.0, -1.0
        job = (np.array([0, 1]), np.array([2]), np.zeros(n_dims), np.ones(n_dims), 1.0)
        out.append(VoteCall("zero_d%d" % n_dims, X, np.array([0, 1, 0]), [job], "linear", None, False))
    return out


def all_vote_calls():
    return vote_calls() + tile_calls() + zero_calls()
