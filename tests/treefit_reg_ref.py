"""A plain NumPy restatement of the regression tree that tree_fit_kernel<best, MSE> (csrc/kernels_treefit.hpp, K19) reproduces:
scikit-learn 1.7.2's DepthFirstTreeBuilder with the squared-error criterion (RegressionCriterion / MSE of _criterion.pyx) over the
BestSplitter, as RandomForestRegressor(n_estimators) fits its trees: max_features = n_dims, min_samples_split = 2,
min_samples_leaf = 1, no depth limit, one output, integer sample weights (0: the row is out of the bag).  The draw, the
candidate rule, the threshold rule and the leaf rules are those of treefit_ref.py; the criterion:
 * per node sum_total = sum w y, sq_sum_total = sum (w y) y, weighted_n = sum w; value = sum_total / weighted_n; the root's
   impurity is sq_sum_total / weighted_n - (sum_total / weighted_n)^2;
 * the proxy at position p of the sorted rows is sum_left^2 / w_left + sum_right^2 / w_right, sum_left the prefix of w y and
   sum_right = sum_total - sum_left; the first strict maximum wins;
 * after the partition sq_sum_left = sum_left (w y) y, sq_sum_right = sq_sum_total - sq_sum_left; a child's impurity is
   sq_sum / w - (sum / w)^2.
Every sum here runs in row order (np.cumsum).  scikit-learn's own order (its introsort and in-place partition) is not restated, and
neither is the kernel's: when the targets and the weights make all sums exact in FP64 -- the cases below: multiples of 1/8,
|y| <= 1024, total weight <= 8192, so sum w y y needs at most 13 + 20 + 6 bits -- the order is immaterial and the three agree bit
for bit.  For other targets check_cart_tree holds a tree to what CART demands, in exact arithmetic."""
from fractions import Fraction

import numpy as np

import treefit_ref as T
from treefit_ref import EPS, RAND_R_MAX, THR32, FixedSeed, bootstrap_weights, forest_seeds, splitter_seed, standardize32  # noqa: F401

TREE_FIELDS = T.TREE_FIELDS
FIELDS = TREE_FIELDS + ("missing_go_to_left",)
MAX_ABS_Y, MAX_WEIGHT_SUM = 1024.0, 8192


def _seq_sum(v):
    return np.float64(np.cumsum(v)[-1]) if v.shape[0] else np.float64(0.0)


def _impurity(sq, s, w):
    return sq / w - (s / w) * (s / w)


def fit_tree(x32, y, weight, seed):
    """One regression tree over the rows of x32 [n][n_dims] (float32) with targets y, integer weights and the rand_r seed.  Returns a
    dict of scikit-learn's tree_ arrays (value as [nodes][1])."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.float64)
    weight = np.asarray(weight).astype(np.int64)
    n_dims = x32.shape[1]
    max_features = n_dims
    rng = T._Rand(seed)
    features = list(range(n_dims))
    constant = [0] * n_dims
    samples = np.flatnonzero(weight != 0)
    w_total = np.float64(weight[samples].sum())
    out = {k: [] for k in FIELDS}
    stack = [(samples, -1, False, None, 0)]
    while stack:
        rows, parent, is_left, impurity, n_known = stack.pop()
        n = rows.shape[0]
        wf = weight[rows].astype(np.float64)
        wy = wf * y[rows]
        sum_total, sq_total, w_node = _seq_sum(wy), _seq_sum(wy * y[rows]), np.float64(weight[rows].sum())
        if impurity is None:
            impurity = _impurity(sq_total, sum_total, w_node)
        is_leaf = n < 2 or impurity <= EPS
        best = None
        if not is_leaf:
            best_proxy = -np.inf
            f_i, n_found, n_drawn, n_total, n_visited = n_dims, 0, 0, n_known, 0
            while f_i > n_total and (n_visited < max_features or n_visited <= n_found + n_drawn):
                n_visited += 1
                f_j = rng.rand_int(n_drawn, f_i - n_found)
                if f_j < n_known:
                    features[n_drawn], features[f_j] = features[f_j], features[n_drawn]
                    n_drawn += 1
                    continue
                f_j += n_found
                f = features[f_j]
                v = x32[rows, f]
                if v.max() <= np.float32(v.min() + THR32):
                    features[f_j], features[n_total] = features[n_total], features[f_j]
                    n_found += 1
                    n_total += 1
                    continue
                f_i -= 1
                features[f_i], features[f_j] = features[f_j], features[f_i]
                order = np.argsort(v, kind="stable")
                sv = v[order]
                sl = np.cumsum(wy[order])[:-1]                  # left of position p = 1 .. n - 1
                wl = np.cumsum(wf[order])[:-1]
                sr = sum_total - sl
                with np.errstate(all="ignore"):
                    proxy = sl * sl / wl + sr * sr / (w_node - wl)
                proxy = np.where(sv[1:] > sv[:-1] + THR32, proxy, -np.inf)
                p = int(np.argmax(proxy))                       # the first maximum
                if proxy[p] > best_proxy:
                    best_proxy = proxy[p]
                    thr = np.float64(sv[p]) / 2.0 + np.float64(sv[p + 1]) / 2.0
                    if thr == np.float64(sv[p + 1]) or np.isinf(thr):
                        thr = np.float64(sv[p])
                    best = (f, thr)
            features[:n_known] = constant[:n_known]
            constant[n_known:n_known + n_found] = features[n_known:n_known + n_found]
            n_known = n_total
            if best is None:
                is_leaf = True
            else:
                go_left = x32[rows, best[0]].astype(np.float64) <= best[1]
                lrows, rrows = rows[go_left], rows[~go_left]
                sum_l, sq_l, wl = _seq_sum(wy[go_left]), _seq_sum(wy[go_left] * y[lrows]), np.float64(weight[lrows].sum())
                wr, sum_r = w_node - wl, sum_total - sum_l
                imp_l, imp_r = _impurity(sq_l, sum_l, wl), _impurity(sq_total - sq_l, sum_r, wr)
                improvement = (w_node / w_total) * (impurity - (wr / w_node * imp_r) - (wl / w_node * imp_l))
                if improvement + EPS < 0.0:
                    is_leaf = True
        node = len(out["feature"])
        if parent >= 0:
            out["children_left" if is_left else "children_right"][parent] = node
        out["children_left"].append(-1)
        out["children_right"].append(-1)
        out["feature"].append(-2 if is_leaf else best[0])
        out["threshold"].append(-2.0 if is_leaf else float(best[1]))
        out["impurity"].append(float(impurity))
        out["n_node_samples"].append(n)
        out["weighted_n_node_samples"].append(float(w_node))
        out["missing_go_to_left"].append(0 if is_leaf else int(lrows.shape[0] > rrows.shape[0]))
        out["value"].append(sum_total / w_node)
        if not is_leaf:
            stack.append((rrows, node, False, imp_r, n_known))
            stack.append((lrows, node, True, imp_l, n_known))
    res = {k: np.asarray(v) for k, v in out.items()}
    res["value"] = res["value"].reshape(-1, 1)
    return res


def sklearn_tree(x32, y, weight, random_state):
    """scikit-learn's own tree for the same problem: DecisionTreeRegressor(random_state) -- squared error, every feature, as the
    estimators of a RandomForestRegressor -- on the float32 rows with the weights as sample_weight."""
    from sklearn.tree import DecisionTreeRegressor
    m = DecisionTreeRegressor(random_state=random_state).fit(np.asarray(x32, dtype=np.float32), np.asarray(y, dtype=np.float64),
                                                             sample_weight=np.asarray(weight, dtype=np.float64))
    t = m.tree_
    res = {k: np.asarray(getattr(t, k)) for k in TREE_FIELDS if k != "value"}
    res["value"] = np.asarray(t.value).reshape(t.node_count, 1)
    res["missing_go_to_left"] = np.asarray(t.missing_go_to_left)
    return res


def assert_exact(y, w):
    """The exactness premise of the goldens: multiples of 1/8 within +-1024, a total weight of at most 8192."""
    y, w = np.asarray(y, dtype=np.float64), np.asarray(w)
    assert np.all(y * 8 == np.round(y * 8)) and np.all(np.abs(y) <= MAX_ABS_Y) and int(w.sum()) <= MAX_WEIGHT_SUM
    assert not np.any(np.signbit(y) & (y == 0))


def eighths(v):
    return np.clip(np.round(np.asarray(v, dtype=np.float64) * 8), -8192, 8192) / 8 + 0.0          # (+ 0.0: no negative zero)


def edge_cases():
    """The small cases of tests/test_treefit_reg_*.py and scripts/make_treefit_reg_golden.py: name -> dict(X, y, w, mean, scale,
    seed), seed being the splitter's rand_r seed.  All targets are multiples of 1/8 within +-1024, every total weight <= 8192."""
    rs = np.random.RandomState(4321)
    out = {}

    def add(name, X, y, w=None, seed=None, standardize=False):
        X = np.asarray(X, dtype=np.float64)
        n, d = X.shape
        w = np.ones(n, dtype=np.int32) if w is None else np.asarray(w, dtype=np.int32)
        y = np.asarray(y, dtype=np.float64)
        assert_exact(y, w)
        mean, scale = (X.mean(0), np.where(X.std(0) > 0, X.std(0), 1.0)) if standardize else (np.zeros(d), np.ones(d))
        out[name] = dict(X=X, y=y, w=w, mean=mean, scale=scale, seed=int(rs.randint(0, RAND_R_MAX)) if seed is None else int(seed))

    def wave(n, d, noise=1.0):
        X = rs.randn(n, d)
        return X, eighths(3.0 * X[:, 0] - 2.0 * np.abs(X[:, d - 1]) + noise * rs.randn(n))

    add("one_in_bag_row", rs.randn(3, 4), [1.5, -2.25, 3.0], w=[0, 1, 0])
    add("two_rows_equal_targets", [[0.0, 1.0], [1.0, 1.0]], [2.5, 2.5])
    add("two_rows_distinct_targets", [[0.0, 1.0], [1.0, 1.0]], [1.0, -3.125])
    add("all_constant", np.ones((12, 5)) * [1.0, -2.0, 0.0, 3.5, 1e-9], np.arange(12) / 8)
    add("constant_target", rs.randn(20, 4), np.full(20, 7.375))
    X, y = wave(60, 5)
    X[:, [0, 2, 4]] = [7.0, -1.0, 0.25]                                   # the draw ends by f_i <= n_total, not by the visit count
    add("three_of_five_constant", X, eighths(y + 4.0 * X[:, 1]))
    X, y = wave(80, 1)
    add("dims_1", X, y, standardize=True)
    X, y = wave(10, 256)
    add("dims_256_few_rows", np.round(X * 512) / 512, y)
    add("integer_ties", rs.randint(0, 4, (200, 6)), eighths(rs.randn(200) * 3))
    # duplicate and adjacent float32 values (FEATURE_THRESHOLD is 0: they split), the smallest denormal next to 0 and the two largest
    # finite values.  The midpoint v[p - 1] / 2.0 + v[p] / 2.0 of two float32 values is exact in FP64, so it never equals v[p]: the
    # threshold fallback cannot be reached from float32 input and stays untested here as in scikit-learn's own suite
    X = np.zeros((40, 3))
    X[:, 0] = np.float32(0.1) + 5e-8 * np.arange(40) + (np.arange(40) >= 20) * 0.1
    X[:, 1] = np.float32(0.3) + 5e-8 * (np.arange(40) % 7)
    f32 = np.finfo(np.float32)
    X[:, 2] = np.array([0.0, f32.smallest_subnormal, float(f32.max), float(np.nextafter(f32.max, np.float32(0))), -f32.smallest_subnormal] * 8,
                       dtype=np.float64)
    add("adjacent_float32_values", X, eighths(rs.randn(40) * 5 + (np.arange(40) % 5) * 3))
    # every split peels the LAST row of the sorted feature off: alternating signs of growing size keep every partial sum small, so
    # the left child is the rest and the pending right children pile up: 599 nodes, 299 of them on the stack at once
    pos = rs.permutation(300)
    add("chain_300", pos.reshape(-1, 1).astype(np.float64), np.where(pos % 2 == 0, 1.0, -1.0) * (pos + 1))
    add("both_signs_at_the_bound", rs.randn(8, 3), [1024.0, -1024.0, 1023.875, -1023.875, 1024.0, -1024.0, 0.125, -0.125], w=[1024] * 8)
    add("one_row_of_weight_8191", rs.randn(5, 2), [-1024.0, 1024.0, 3.5, 0.0, -7.125], w=[1, 8191, 0, 0, 0])
    for n in (63, 64, 65, 255, 256, 257, 513):                           # around the wave, the workgroup and two rows per thread
        X, y = wave(n, 4)
        add("rows_%d" % n, X, y, w=bootstrap_weights(n, n), standardize=True)
    X, y = wave(260, 9)
    add("bootstrap_260x9", X, y, w=bootstrap_weights(3, 260), standardize=True)
    return out


def limit_case(n=8192):
    """The row limit exactly: n in-bag rows of weight 1 (the weight bound), 4 dims of coarse float32 values, targets of a few levels."""
    rs = np.random.RandomState(99)
    X = np.round(rs.randn(n, 4) * 16).astype(np.float64) / 8
    y = eighths(np.round(2.0 * X[:, 0] - X[:, 3] + rs.randn(n) * 0.5) * 64)
    return dict(X=X, y=y, w=np.ones(n, dtype=np.int32), mean=np.zeros(4), scale=np.ones(4), seed=20240229)


def sweep_case():
    """A sweep over 200 x 9 rows: 6 jobs with n_estimators 1 .. 7, one of them with a single test row.  Returns (X, y, jobs) with jobs
    of (train_idx, test_idx, mean, scale, (n_estimators, seed))."""
    rs = np.random.RandomState(78)
    n, d = 200, 9
    X = rs.randn(n, d)
    y = eighths(4.0 * X[:, 0] - 3.0 * X[:, 4] * X[:, 1] + rs.randn(n))
    jobs = []
    for j, ne in enumerate((1, 2, 3, 5, 7, 4)):
        perm = rs.permutation(n)
        n_train = 199 if j == 5 else 180
        tr, te = perm[:n_train], perm[n_train:]
        jobs.append((tr, te, X[tr].mean(0), X[tr].std(0), (ne, int(rs.randint(np.iinfo(np.int32).max)))))
    return X, y, jobs


def sklearn_forest(X, y, job):
    """(predict of the test rows, predict of the training rows, the fitted forest) of scikit-learn's RandomForestRegressor for one job."""
    from sklearn.ensemble import RandomForestRegressor
    tr, te, mean, scale, (ne, seed) = job
    m = RandomForestRegressor(n_estimators=ne, random_state=seed).fit((X[tr] - mean) / scale, y[tr])
    return m.predict((X[te] - mean) / scale), m.predict((X[tr] - mean) / scale), m


def general_case(n=300, d=9, seed=5):
    """Gaussian features (no constant column, no ties) and Gaussian targets: the sums round, so there is no equality to scikit-learn."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, d)
    y = 2.0 * X[:, 0] - X[:, 1] * X[:, 2] + rs.randn(n)
    return X, y


U = Fraction(1, 2 ** 52)


def check_cart_tree(tree, x32, y, weight, distinct=False):
    """Walks a regression tree with exact arithmetic and asserts what CART demands of it (u = 2^-52, sums over a node's rows):
     * n_node_samples and weighted_n_node_samples are exact;
     * value is within n u max|y| of the exact weighted mean;
     * an internal node's (feature, threshold) is a candidate of its rows, the threshold obeys the midpoint rule for its two
       neighbours, and its exact proxy is within 8 n u (sum w |y|)^2 of the exact maximum over all candidates of all features
       (recursive summation errs by at most n u' sum |w y| per sum, u' = u / 2; through the two squares and the divisions by
       weights >= 1 that is below 4 n u (sum w |y|)^2 per proxy, twice that between two of them);
     * a leaf is unsplittable (fewer than 2 rows, or every feature constant on it) or its exact impurity is at most
       DBL_EPSILON + 4 n u max y^2;
     * distinct: every leaf holds one row, predicted as its own target within u max|y|.
    Returns the number of internal nodes."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.float64)
    weight = np.asarray(weight).astype(np.int64)
    yf = [Fraction(float(v)) for v in y]
    n_dims, internal = x32.shape[1], 0
    stack = [(0, np.flatnonzero(weight != 0))]
    while stack:
        node, rows = stack.pop()
        n = rows.shape[0]
        W = int(weight[rows].sum())
        S = sum(int(weight[i]) * yf[i] for i in rows)
        Q = sum(int(weight[i]) * yf[i] * yf[i] for i in rows)
        A = sum(int(weight[i]) * abs(yf[i]) for i in rows)
        ymax = max(abs(yf[i]) for i in rows)
        assert int(tree["n_node_samples"][node]) == n and float(tree["weighted_n_node_samples"][node]) == float(W), node
        assert abs(Fraction(float(tree["value"][node][0])) - S / W) <= n * U * ymax, node
        if int(tree["children_left"][node]) < 0:
            assert int(tree["children_right"][node]) < 0 and int(tree["feature"][node]) == -2
            splittable = n >= 2 and any(x32[rows, f].max() > x32[rows, f].min() for f in range(n_dims))
            assert not splittable or Q / W - (S / W) ** 2 <= Fraction(EPS) + 4 * n * U * ymax * ymax, node
            if distinct:
                assert n == 1 and abs(Fraction(float(tree["value"][node][0])) - yf[rows[0]]) <= U * ymax, node
            continue
        internal += 1
        f, thr = int(tree["feature"][node]), float(tree["threshold"][node])
        best, chosen = None, None
        for g in range(n_dims):
            order = np.argsort(x32[rows, g], kind="stable")
            sv, srows = x32[rows, g][order], rows[order]
            sl, wl = Fraction(0), 0
            for p in range(1, n):
                i = srows[p - 1]
                sl, wl = sl + int(weight[i]) * yf[i], wl + int(weight[i])
                if not sv[p] > sv[p - 1]:
                    continue
                proxy = sl * sl / wl + (S - sl) * (S - sl) / (W - wl)
                best = proxy if best is None or proxy > best else best
                if g == f and np.float64(sv[p - 1]) <= thr < np.float64(sv[p]):
                    mid = np.float64(sv[p - 1]) / 2.0 + np.float64(sv[p]) / 2.0
                    assert thr == (np.float64(sv[p - 1]) if mid == np.float64(sv[p]) or np.isinf(mid) else mid), node
                    chosen = proxy
        assert chosen is not None, (node, f, thr)                      # a candidate of the node's rows
        assert best - chosen <= 8 * n * U * A * A, (node, float(best - chosen))
        go_left = x32[rows, f].astype(np.float64) <= thr
        assert int(tree["missing_go_to_left"][node]) == int(go_left.sum() > n - go_left.sum())
        stack.append((int(tree["children_right"][node]), rows[~go_left]))
        stack.append((int(tree["children_left"][node]), rows[go_left]))
    return internal


CHUNK_TREES = 700
CHUNK_LAYOUT, CHUNK_TINY, CHUNK_NO_TEST = T.CHUNK_LAYOUT, T.CHUNK_TINY, T.CHUNK_NO_TEST


def chunk_sweep_case():
    """The regressor's sweep over three chunks of the real 1 GiB bound: the rows, lists, means and scales of
    treefit_ref.chunk_sweep_case with 700 trees per big job (a tree of ~5180 in-bag rows takes ~0.53 MB of capacity, whatever its
    depth).  The targets are the cell of the 8 x 8 grid the row lies in -- 64 levels a tree finds with a few exact cuts -- plus noise on
    every 16th row, which the tree must then isolate: ~1/6 of the nodes of an unrestricted target, so that the ~10 000 trees of the test
    stay within seconds.  Multiples of 1/8 within +-1024 and a bootstrap's total weight of 8192: every sum is exact."""
    X, _, jobs = T.chunk_sweep_case("randomforest")
    rs = np.random.RandomState(707)
    cell = 8.0 * np.floor(np.clip(X[:, 0], 0, 7.5)) + np.floor(np.clip(X[:, 1], 0, 7.5))
    y = eighths(cell + np.where(np.arange(X.shape[0]) % 16 == 0, 4.0 * rs.randn(X.shape[0]), 0.0))
    jobs = [j[:4] + ((j[4][0] if i == CHUNK_TINY else CHUNK_TREES, j[4][1]),) for i, j in enumerate(jobs)]
    for j in jobs:
        assert_exact(y[j[0]], np.ones(len(j[0]), dtype=np.int64))
    return X, y, jobs


def many_test_rows_case():
    """One job whose test list is longer than one traversal pass of the sweep's scoring (32 768 rows): 60 training rows, 3 trees,
    32 769 + 5 test rows of a 33 000 x 3 matrix.  Returns (X, labels of 3 classes, exact targets, the job)."""
    rs = np.random.RandomState(808)
    X = np.round(rs.randn(33000, 3) * 64) / 64
    labels = (np.arange(33000) % 3).astype(np.float64)
    X[:, 0] += labels
    y = eighths(3.0 * X[:, 0] - 2.0 * np.abs(X[:, 2]) + rs.randn(33000))
    tr, te = np.arange(60), 60 + rs.permutation(32940)[:32769 + 5]
    return X, labels, y, (tr, te, X[tr].mean(0), X[tr].std(0), (3, 90210))
