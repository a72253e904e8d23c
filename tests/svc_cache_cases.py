"""The inputs of the tests of the C-SVC solver's resident kernel matrices (DESIGN K23), shared by tests/test_svc_cache_cpu.py
(which asserts, without a device, that the inputs make the sizes, shared rows, duplicates and non-monotone position lists they are
meant to make, and holds the library's layout against the restatement) and tests/test_svc_cache_gpu.py (which runs them under
kernel_cache="none" and "gram" and asks for the same bytes).  Plain NumPy; imports nothing from the package.

A solver task is what audioTrainTest.smo_solve takes: (rows, signs, mean, scale, C, gamma)."""
import functools

import numpy as np

DIMS = (1, 9, 136, 256)
SIZE_ROWS = (1, 2, 255, 256, 257, 513)      # smo_cached_kernel runs one thread per row, 256 threads: its stride's edges
N_SAMPLES = 1400
THREE_CLASSES = (90, 70, 50)
FOLD_PAIR = (70, 50)                        # the rows of the two classes of the pair whose folds are restated
EPS = 1e-3
MAX_ROWS = 8192


def matrix_bytes(n):
    return 8 * int(n) * int(n)


@functools.lru_cache(maxsize=None)
def samples(n_dims):
    """(X [1400][n_dims], y [1400]): two overlapping Gaussian classes in alternation on features of unequal scale."""
    rng = np.random.default_rng(4100 + n_dims)
    y = np.where(np.arange(N_SAMPLES) % 2 == 0, 1.0, -1.0)
    X = rng.standard_normal((N_SAMPLES, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    X += 1.2 * y[:, None] / np.sqrt(n_dims)
    return X, y


def _stats(X, rows):
    mean, scale = X[rows].mean(axis=0), X[rows].std(axis=0)
    return mean, np.where(scale > 0, scale, 1.0)


def fold_like(rng, n, signs):
    """Five subsets of 0 .. n - 1 as libsvm's folds make them: a permutation, fold f leaves its fifth out, the rest in
    permutation order grouped by sign, the sign seen first put first."""
    perm = rng.permutation(n)
    out = []
    for f in range(5):
        begin, end = f * n // 5, (f + 1) * n // 5
        kept = np.concatenate([perm[:begin], perm[end:]])
        lead = signs[kept[0]]
        out.append(np.concatenate([kept[signs[kept] == lead], kept[signs[kept] != lead]]))
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch(n_dims):
    """(X, tasks, groups, names): one call's worth of tasks over samples(n_dims).
    size<n>       a task of n rows for every n of SIZE_ROWS, each its own group with the statistics of its own rows;
    three_ab ..   the three pair tasks of three classes of 90, 70 and 50 samples, one group: the tasks share rows;
    pair, fold0.. a pair task of 70 + 50 rows and five fold-like permuted subsets of it, one group: the position lists of the
                  folds are not monotone;
    twice         a task that lists one sample twice, with the same sign, its own group;
    gamma_a/b     two groups of two tasks each over the same rows, with different gammas (read by the RBF kernel)."""
    X, y = samples(n_dims)
    rng = np.random.default_rng(4200 + n_dims)
    tasks, groups, names = [], [], []
    gid = 0
    for n in SIZE_ROWS:
        rows = rng.permutation(N_SAMPLES)[:n]
        if n == 2:
            rows = np.array([10, 11])            # one row of either sign
        mean, scale = _stats(X, rows) if n > 1 else (np.zeros(n_dims), np.ones(n_dims))
        tasks.append((rows, y[rows], mean, scale, 0.05 if n == 513 else 1.0, None))     # (the longest task at a C that keeps it short)
        groups.append(gid)
        names.append("size%d" % n)
        gid += 1
    # three classes of samples drawn from 100 .. 999: a class is no sign here -- the pair decides the signs
    cls = []
    pool = 100 + rng.permutation(900)
    at = 0
    for n in THREE_CLASSES:
        cls.append(np.sort(pool[at:at + n]))
        at += n
    Xc = X.copy()
    for c in range(3):                           # pull the classes apart a little, whatever y says of their rows
        Xc[cls[c]] += (c - 1) * 0.8 / np.sqrt(n_dims)
    all3 = np.concatenate(cls)
    mean, scale = _stats(Xc, all3)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        rows = np.concatenate([cls[a], cls[b]])
        tasks.append((rows, np.concatenate([np.ones(len(cls[a])), -np.ones(len(cls[b]))]), mean, scale, 2.0, 0.4 / n_dims))
        groups.append(gid)
        names.append("three_%d%d" % (a, b))
    gid += 1
    # a pair and its folds
    pa, pb = 1000 + np.arange(FOLD_PAIR[0]), 1100 + np.arange(FOLD_PAIR[1])
    rows = np.concatenate([pa, pb])
    signs = np.concatenate([np.ones(len(pa)), -np.ones(len(pb))])
    Xc[pa] += 0.5 / np.sqrt(n_dims)
    mean, scale = _stats(Xc, rows)
    tasks.append((rows, signs, mean, scale, 1.0, None))
    groups.append(gid)
    names.append("pair")
    for f, sub in enumerate(fold_like(rng, len(rows), signs)):
        tasks.append((rows[sub], signs[sub], mean, scale, 1.0, None))
        groups.append(gid)
        names.append("fold%d" % f)
    gid += 1
    # one sample twice
    rows = np.array([1200, 1201, 1202, 1203, 1200, 1204, 1205, 1206, 1207])
    tasks.append((rows, y[rows], *_stats(Xc, rows[:4]), 1.0, None))
    groups.append(gid)
    names.append("twice")
    gid += 1
    # two gammas
    ga = 1250 + np.arange(60)
    gb = ga[::-1][:41]
    mean, scale = _stats(Xc, ga)
    for name, gamma in (("gamma_a", 0.1 / n_dims), ("gamma_b", 2.0 / n_dims)):
        for k, rows in enumerate((ga, gb)):
            tasks.append((rows, y[rows], mean, scale, 5.0, gamma))
            groups.append(gid)
            names.append("%s%d" % (name, k))
        gid += 1
    return Xc, tasks, np.array(groups, dtype=np.int32), names


def group_sizes(tasks, groups):
    """{group id: distinct samples}, ids in order of first appearance."""
    out = {}
    for task, g in zip(tasks, groups):
        out.setdefault(int(g), set()).update(int(r) for r in task[0])
    return {g: len(s) for g, s in out.items()}


# hand-counted layouts: (task rows, groups, budget, group_of, group rows, pos, chunk)
LAYOUTS_BY_HAND = (
    # two tasks share the samples 7 and 9; the second lists 7 twice; first appearance decides the order
    (([9, 7, 4], [7, 2, 7, 9]), (5, 5), 8 * 16, [0, 0], [[9, 7, 4, 2]], [[0, 1, 2], [1, 3, 1, 0]], [0]),
    # the same under a budget one byte short: the group is not cached
    (([9, 7, 4], [7, 2, 7, 9]), (5, 5), 8 * 16 - 1, [0, 0], [[9, 7, 4, 2]], [[0, 1, 2], [1, 3, 1, 0]], [-1]),
    # groups are numbered by first appearance, not by id; a group of one task of one row; no ids: every task its own group
    (([3, 1], [8], [1, 5]), (9, 2, 9), 8 * 9 + 8, [0, 1, 0], [[3, 1, 5], [8]], [[0, 1], [0], [1, 2]], [0, 0]),
    (([3, 1], [8], [1, 5]), (9, 2, 9), 8 * 9, [0, 1, 0], [[3, 1, 5], [8]], [[0, 1], [0], [1, 2]], [0, 1]),
    (([3, 1], [8], [1, 5]), None, 8 * 5, [0, 1, 2], [[3, 1], [8], [1, 5]], [[0, 1], [0], [0, 1]], [0, 0, 1]),
    # a group in the middle exceeds the budget alone: the groups around it share a chunk
    (([0, 1], [0, 1, 2, 3], [4, 5]), (0, 1, 2), 8 * 8, [0, 1, 2], [[0, 1], [0, 1, 2, 3], [4, 5]], [[0, 1], [0, 1, 2, 3], [0, 1]], [0, -1, 0]),
)


def random_layout_case(seed):
    """(task rows, groups or None, budget) of a seeded random sweep for the layout alone."""
    rng = np.random.default_rng([91, seed])
    n_tasks = int(rng.integers(1, 12))
    n_samples = int(rng.integers(1, 40))
    rows = [rng.integers(0, n_samples, int(rng.integers(1, 30))) for _ in range(n_tasks)]
    groups = None if seed % 4 == 0 else rng.integers(-3, 4, n_tasks)
    budget = int(rng.integers(1, 8 * n_samples * n_samples + 2))
    return rows, groups, budget


def big_groups():
    """(X, tasks, groups): nine groups of 8192 distinct rows x 1 dim, each a task over all its rows and a permuted half of them:
    under a budget of 5 GiB one chunk of 4.5 GiB, so the last group's matrix begins at byte offset 4 GiB."""
    rng = np.random.default_rng(78)
    n = MAX_ROWS
    X = rng.standard_normal((n + 500, 1))
    y = np.where(X[:, 0] + 0.8 * rng.standard_normal(n + 500) > 0, 1.0, -1.0)
    tasks, groups = [], []
    for k in range(9):
        rows = rng.permutation(n + 500)[:n]
        mean, scale = np.array([0.1 * k]), np.array([1.0 + 0.05 * k])
        half = rows[rng.permutation(n)[:n // 2]]
        for r in (rows, half):
            tasks.append((r, y[r], mean, scale, 0.5 + k, 0.3 + 0.1 * k))
            groups.append(k)
    return X, tasks, np.array(groups, dtype=np.int32)
