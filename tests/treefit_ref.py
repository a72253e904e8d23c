"""A plain NumPy restatement of the tree builder that tree_fit_kernel (csrc/kernels_treefit.hpp) reproduces: scikit-learn
1.7.2's DepthFirstTreeBuilder with the Gini criterion, BestSplitter ("randomforest") or RandomSplitter ("extratrees"),
max_features = max(1, int(sqrt(n_dims))), min_samples_split = 2, min_samples_leaf = 1, no depth limit, no missing values,
integer sample weights (0: the row is out of the bag).  Written from the rules, not for speed: tests use it at small shapes.

The rules that decide equality:
 * x32 = float32((x - mean) / scale); rows of weight 0 are not part of the tree;
 * rand_r: 32-bit xorshift 13 / 17 / 5, seed 0 replaced by 1, result modulo 2^31; rand_int = low + r % (high - low);
   rand_uniform = (high - low) * r / 2147483647.0 + low in FP64;
 * the Fisher-Yates feature draw with the drawn / known / found constant bookkeeping; `features` persists over the nodes of a
   tree, `constant_features` is one array whose prefix belongs to the node being split;
 * FEATURE_THRESHOLD is 0: _partitioner.pxd declares 1e-7, but the initialiser of a cdef variable in a .pxd takes no effect and
   the compiled 1.7.2 compares against 0 (it splits adjacent float32 values); a feature is constant in a node when max <= min;
 * best splitter: the candidates are the positions p of the sorted values with v[p] > v[p - 1]; the proxy is
   -w_right * gini_right - w_left * gini_left with gini = 1 - sum_k count_k^2 / (w * w), strict >; the threshold is
   v[p - 1] / 2.0 + v[p] / 2.0 in FP64, v[p - 1] when that equals v[p] or is infinite;
 * random splitter: threshold = rand_uniform(min, max), min when it equals max; left: x32 <= threshold;
 * a node is a leaf when it has fewer than 2 rows, its impurity is <= DBL_EPSILON, no split was found, or the split's
   improvement + DBL_EPSILON < 0;
 * nodes are numbered in preorder (left subtree first); value = counts / weighted count.
Nothing depends on the order of the rows inside a node: the class statistics are sums of integers."""
import numpy as np

RAND_R_MAX = 2147483647
EPS = float(np.finfo(np.float64).eps)
THR32 = np.float32(0.0)


class _Rand:
    def __init__(self, seed):
        self.s = int(seed) & 0xFFFFFFFF

    def next(self):
        s = self.s
        if s == 0:
            s = 1
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        self.s = s
        return s % (RAND_R_MAX + 1)

    def rand_int(self, low, high):
        return low + self.next() % (high - low)

    def rand_uniform(self, low, high):
        return (np.float64(high) - np.float64(low)) * np.float64(self.next()) / np.float64(RAND_R_MAX) + np.float64(low)


def _gini(counts, w):
    sq = np.float64(0.0)
    for c in counts:
        sq = sq + np.float64(c) * np.float64(c)
    return np.float64(1.0) - sq / (np.float64(w) * np.float64(w))


def _proxy(left, right, wl, wr):
    return -np.float64(wr) * _gini(right, wr) - np.float64(wl) * _gini(left, wl)


def standardize32(X, mean, scale):
    return ((np.asarray(X, dtype=np.float64) - mean) / scale).astype(np.float32)


def fit_tree(x32, y, weight, n_classes, seed, splitter):
    """One tree over the rows of x32 [n][n_dims] (float32) with class indices y, integer weights and the rand_r seed; splitter
    "best" or "random".  Returns a dict of scikit-learn's tree_ arrays (value as [nodes][n_classes])."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    weight = np.asarray(weight).astype(np.int64)
    n_dims = x32.shape[1]
    max_features = max(1, int(np.sqrt(n_dims)))
    rng = _Rand(seed)
    features = list(range(n_dims))
    constant = [0] * n_dims
    samples = np.flatnonzero(weight != 0)
    w_total = np.float64(weight[samples].sum())
    out = {k: [] for k in ("children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples",
                           "weighted_n_node_samples", "missing_go_to_left", "value")}

    def counts_of(rows):
        return np.bincount(y[rows], weights=weight[rows], minlength=n_classes).astype(np.int64)

    stack = [(samples, -1, False, None, 0)]
    while stack:
        rows, parent, is_left, impurity, n_known = stack.pop()
        n = rows.shape[0]
        total = counts_of(rows)
        w_node = int(total.sum())
        if impurity is None:
            impurity = _gini(total, w_node)
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
                lo, hi = v.min(), v.max()
                if hi <= np.float32(lo + THR32):
                    features[f_j], features[n_total] = features[n_total], features[f_j]
                    n_found += 1
                    n_total += 1
                    continue
                f_i -= 1
                features[f_i], features[f_j] = features[f_j], features[f_i]
                if splitter == "best":
                    order = np.argsort(v, kind="stable")
                    sv, srows = v[order], rows[order]
                    left = np.zeros(n_classes, dtype=np.int64)
                    for p in range(1, n):
                        left[y[srows[p - 1]]] += weight[srows[p - 1]]
                        if sv[p] <= np.float32(sv[p - 1] + THR32):
                            continue
                        wl = int(left.sum())
                        proxy = _proxy(left, total - left, wl, w_node - wl)
                        if proxy > best_proxy:
                            best_proxy = proxy
                            thr = np.float64(sv[p - 1]) / 2.0 + np.float64(sv[p]) / 2.0
                            if thr == np.float64(sv[p]) or np.isinf(thr):
                                thr = np.float64(sv[p - 1])
                            best = (f, thr)
                else:
                    thr = rng.rand_uniform(lo, hi)
                    if thr == np.float64(hi):
                        thr = np.float64(lo)
                    go_left = v.astype(np.float64) <= thr
                    n_left = int(go_left.sum())
                    if n_left < 1 or n - n_left < 1:
                        continue
                    left = counts_of(rows[go_left])
                    wl = int(left.sum())
                    proxy = _proxy(left, total - left, wl, w_node - wl)
                    if proxy > best_proxy:
                        best_proxy = proxy
                        best = (f, thr)
            features[:n_known] = constant[:n_known]
            constant[n_known:n_known + n_found] = features[n_known:n_known + n_found]
            n_known = n_total
            if best is None:
                is_leaf = True
            else:
                go_left = x32[rows, best[0]].astype(np.float64) <= best[1]
                lrows, rrows = rows[go_left], rows[~go_left]
                left = counts_of(lrows)
                right = total - left
                wl = int(left.sum())
                wr = w_node - wl
                imp_l, imp_r = _gini(left, wl), _gini(right, wr)
                improvement = (np.float64(w_node) / w_total) * (impurity - (np.float64(wr) / np.float64(w_node) * imp_r)
                                                                - (np.float64(wl) / np.float64(w_node) * imp_l))
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
        out["value"].append(total.astype(np.float64) / np.float64(w_node))
        if not is_leaf:
            stack.append((rrows, node, False, imp_r, n_known))
            stack.append((lrows, node, True, imp_l, n_known))
    res = {k: np.asarray(v) for k, v in out.items()}
    res["value"] = res["value"].reshape(-1, n_classes)
    return res


TREE_FIELDS = ("children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted_n_node_samples",
               "value")


def sklearn_tree(x32, y, weight, n_classes, random_state, splitter):
    """scikit-learn's own tree for the same problem: DecisionTreeClassifier / ExtraTreeClassifier(max_features="sqrt",
    random_state) on the float32 rows with the weights as sample_weight.  Returns (the arrays of TREE_FIELDS and
    missing_go_to_left, the rand_r seed the splitter drew).  y must hold every class 0 .. n_classes - 1 in its weighted
    rows or the value width differs."""
    from sklearn.tree import DecisionTreeClassifier, ExtraTreeClassifier
    cls = DecisionTreeClassifier if splitter == "best" else ExtraTreeClassifier
    m = cls(max_features="sqrt", random_state=random_state).fit(np.asarray(x32, dtype=np.float32), y,
                                                               sample_weight=np.asarray(weight, dtype=np.float64))
    t = m.tree_
    res = {k: np.asarray(getattr(t, k)) for k in TREE_FIELDS if k != "value"}
    res["value"] = np.asarray(t.value).reshape(t.node_count, -1)
    res["missing_go_to_left"] = np.asarray(t.missing_go_to_left)
    if isinstance(random_state, np.random.RandomState):        # (a FixedSeed: the state is not consumed)
        return res, int(random_state.randint(0, RAND_R_MAX))
    return res, int(np.random.RandomState(random_state).randint(0, RAND_R_MAX))


def forest_seeds(random_state, n_estimators):
    """Per tree the random_state scikit-learn's forests give their estimators: one randint(MAX_INT) each, in order."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    return [int(rs.randint(np.iinfo(np.int32).max)) for _ in range(n_estimators)]


def bootstrap_weights(seed, n):
    return np.bincount(np.random.RandomState(seed).randint(0, n, n, dtype=np.int32), minlength=n)


def splitter_seed(seed):
    return int(np.random.RandomState(seed).randint(0, RAND_R_MAX))


def _unstep(s):
    """The rand_r state before the one that gives s (the xorshift steps inverted)."""
    def unshift_left(v, k):
        r = v
        for _ in range(32 // k + 1):
            r = v ^ ((r << k) & 0xFFFFFFFF)
        return r

    def unshift_right(v, k):
        r = v
        for _ in range(32 // k + 1):
            r = v ^ (r >> k)
        return r
    return unshift_left(unshift_right(unshift_left(s, 5), 17), 13)


def seed_with_draw(value, after):
    """A rand_r seed whose draw number `after` (from 0) leaves the state `value`: 0xffffffff draws RAND_R_MAX."""
    s = value
    for _ in range(after + 1):
        s = _unstep(s)
    return s


class FixedSeed(np.random.RandomState):
    """A RandomState whose randint returns one fixed value: hands scikit-learn's splitter a chosen rand_r seed."""

    def __init__(self, value):
        super().__init__(0)
        self.value = int(value)

    def randint(self, *args, **kwargs):
        return self.value


def edge_cases():
    """The small cases of tests/test_treefit_*.py and scripts/make_treefit_golden.py: name -> dict(X, y, w, mean, scale, seed), seed
    being the splitter's rand_r seed.  Each is fitted with both splitters.  y holds every class in a weighted row."""
    rs = np.random.RandomState(1234)
    out = {}

    def add(name, X, y, w=None, seed=None, standardize=False):
        X = np.asarray(X, dtype=np.float64)
        n, d = X.shape
        w = np.ones(n, dtype=np.int32) if w is None else np.asarray(w, dtype=np.int32)
        mean, scale = (X.mean(0), np.where(X.std(0) > 0, X.std(0), 1.0)) if standardize else (np.zeros(d), np.ones(d))
        out[name] = dict(X=X, y=np.asarray(y, dtype=np.int64), w=w, mean=mean, scale=scale,
                         seed=int(rs.randint(0, RAND_R_MAX)) if seed is None else int(seed))

    def blobs(n, d, k, spread=0.6):
        y = np.arange(n) % k
        rs.shuffle(y)
        return rs.randn(n, d) + spread * y[:, None] * rs.randn(1, d), y

    add("one_in_bag_row", rs.randn(3, 4), [0, 1, 0], w=[0, 1, 0])
    add("one_class", rs.randn(20, 4), np.zeros(20))
    add("two_rows", [[0.0, 1.0], [1.0, 1.0]], [0, 1])
    add("all_constant", np.ones((12, 5)) * [1.0, -2.0, 0.0, 3.5, 1e-9], np.arange(12) % 3)
    X, y = blobs(60, 5, 3)
    X[:, [0, 2, 4]] = [7.0, -1.0, 0.25]
    add("three_of_five_constant", X, y)
    add("integer_ties", rs.randint(0, 4, (200, 6)), rs.randint(0, 3, 200))
    X = np.zeros((40, 2))
    X[:, 0] = np.float32(0.1) + 5e-8 * np.arange(40) + (np.arange(40) >= 20) * 0.1       # steps below the declared 1e-7 (scikit-learn 1.7.2 splits them all the same), one gap
    X[:, 1] = np.float32(0.3) + 5e-8 * (np.arange(40) % 7)
    add("values_5e-8_apart", X, np.arange(40) % 2)
    X = np.array([[3e38, 1.0], [2.9e38, 2.0], [-3e38, 3.0], [-2.9e38, 4.0], [3.3e38, 5.0], [-3.3e38, 6.0], [1e38, 7.0], [-1e38, 8.0]] * 2)
    X[8:, 1] += 0.5
    add("values_near_3e38", X, [0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1])
    X, y = blobs(100, 6, 3)
    add("weights_0_1_2", X, y, w=np.maximum(rs.randint(0, 4, 100), (np.arange(100) < 3).astype(int)), standardize=True)
    for n in (63, 64, 65, 255, 256, 257):
        X, y = blobs(n, 4, 3)
        add("rows_%d" % n, X, y, standardize=True)
    X = rs.permutation(300).reshape(-1, 1).astype(np.float64)
    add("chain_300", X, X[:, 0].astype(np.int64) % 2)          # labels alternate along the sorted feature: depth near the row count
    for k in (2, 8, 64):
        X, y = blobs(200, 6, k, spread=0.2)
        add("classes_%d" % k, X, y, standardize=True)
    for d in (1, 136, 138):
        X, y = blobs(80, d, 3)
        add("dims_%d" % d, np.round(X * 512) / 512, y, standardize=True)
    X, y = blobs(260, 136, 8, spread=0.3)
    add("bootstrap_260x136", np.round(X * 512) / 512, y, w=bootstrap_weights(3, 260), standardize=True)
    # extra trees: the root's threshold draw (draw 1, after the feature draw) returns RAND_R_MAX, so the threshold equals the maximum
    add("threshold_equals_max", np.array([[0.0], [1.0], [2.0], [3.0], [1.0], [3.0]]), [0, 1, 0, 1, 1, 0], seed=seed_with_draw(0xFFFFFFFF, 1))
    return out


def limit_case(n=8192):
    """The row limit exactly: n rows, 2 dims, 2 overlapping classes, every value a float32 (so the file compresses)."""
    rs = np.random.RandomState(99)
    y = np.arange(n) % 2
    X = np.round(rs.randn(n, 2) * 64 + y[:, None] * 24).astype(np.float64) / 8
    return dict(X=X, y=y.astype(np.int64), w=np.ones(n, dtype=np.int32), mean=np.zeros(2), scale=np.ones(2), seed=20240229)


def wide_limit_case(n_classes=64, n=8192):
    """The classifier's largest launch: the row limit with 64 classes (128 histogram columns of 64 rows) or, with n_classes=32, the
    same rows labelled y % 32 (the full 32 x 257 histogram, the column switch from below).  3 dims, every value a float32 multiple
    of 1/64: columns 0 and 1 are the class's place on an 8 x 8 grid plus noise, column 2 is noise.  Weights: mostly 1, 400 rows 0,
    300 rows 3, one row 8191 (the weight limit); every class keeps a weighted row.  scikit-learn 1.7.2 grows 8089 (best) and 12351
    (random) nodes on the 64 classes."""
    rs = np.random.RandomState(2025)
    y = np.arange(n) % 64
    rs.shuffle(y)
    X = np.stack([y % 8 + 0.4 * rs.randn(n), y // 8 + 0.4 * rs.randn(n), rs.randn(n)], axis=1)
    X = (np.round(X * 64) / 64).astype(np.float32).astype(np.float64)
    w = np.ones(n, dtype=np.int32)
    pick = rs.permutation(n)
    w[pick[:400]], w[pick[400:700]], w[pick[700]] = 0, 3, 8191
    y = (y % n_classes).astype(np.int64)
    assert np.unique(y[w > 0]).shape[0] == n_classes
    return dict(X=X, y=y, w=w, mean=np.zeros(3), scale=np.ones(3), seed=20250611)


def sweep_case():
    """A sweep of 3 classes over 330 rows: n_estimators 1, 3, 10 x 2 experiments, plus one job whose training list lacks class 2.
    Returns (X, y, jobs) with jobs of (train_idx, test_idx, mean, scale, (n_estimators, seed))."""
    rs = np.random.RandomState(77)
    n, d, k = 330, 20, 3
    y = (np.arange(n) % k).astype(np.float64)
    X = rs.randn(n, d) + 0.5 * y[:, None] * rs.randn(1, d)
    jobs = []
    for ne in (1, 3, 10):
        for _ in range(2):
            perm = rs.permutation(n)
            tr, te = perm[:297], perm[297:]
            jobs.append((tr, te, X[tr].mean(0), X[tr].std(0), (ne, int(rs.randint(np.iinfo(np.int32).max)))))
    tr = np.flatnonzero(y != 2)[:150]
    te = np.arange(n)[-30:]
    jobs.append((tr, te, X[tr].mean(0), X[tr].std(0), (5, 4242)))
    return X, y, jobs


def sklearn_forest(X, y, job, kind):
    """(predict, predict_proba, the fitted forest) of scikit-learn's forest for one job of sweep_case."""
    from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
    tr, te, mean, scale, (ne, seed) = job
    cls = RandomForestClassifier if kind == "randomforest" else ExtraTreesClassifier
    m = cls(n_estimators=ne, random_state=seed).fit((X[tr] - mean) / scale, y[tr])
    Z = (X[te] - mean) / scale
    return m.predict(Z), m.predict_proba(Z), m


def dims_and_weight_cases():
    """The classifier's remaining edges, held by fit_tree (tests/test_treefit_scale_*.py): 255 and 256 dims (max_features 15 and 16;
    256 is the dims limit, the two feature arrays full) and the weight limit 8191 among the weights 0, 1, 2."""
    rs = np.random.RandomState(4711)
    out = {}
    for d in (255, 256):
        y = np.arange(80) % 3
        rs.shuffle(y)
        X = np.round((rs.randn(80, d) + 0.6 * y[:, None] * rs.randn(1, d)) * 512) / 512
        out["dims_%d" % d] = dict(X=X, y=y.astype(np.int64), w=np.ones(80, dtype=np.int32), mean=X.mean(0), scale=X.std(0),
                                  seed=int(rs.randint(0, RAND_R_MAX)))
    y = np.arange(100) % 3
    rs.shuffle(y)
    X = rs.randn(100, 4) + 0.6 * y[:, None] * rs.randn(1, 4)
    w = np.array([0, 1, 2, 8191], dtype=np.int32)[rs.randint(0, 4, 100)]
    first = [int(np.flatnonzero(y == c)[0]) for c in range(3)]
    w[first] = np.maximum(w[first], 1)                                              # every class keeps a weighted row
    assert np.unique(y[w > 0]).shape[0] == 3 and set(w.tolist()) == {0, 1, 2, 8191}
    out["weights_0_1_2_8191"] = dict(X=X, y=y.astype(np.int64), w=w, mean=np.zeros(4), scale=np.ones(4), seed=int(rs.randint(0, RAND_R_MAX)))
    return out


def check_gini_tree(tree, x32, y, weight, n_classes):
    """Walks a classification tree on the host and asserts what holds of EVERY tree the builder may return for these rows, whichever
    features it drew: n_node_samples and weighted_n_node_samples are the true counts of the rows that reach the node; value is the
    weighted class fraction of those rows (integer counts, one FP64 division: exact to the bit); impurity is the Gini of those counts
    in class order; an internal node sends at least one row each way and its missing_go_to_left names the larger side; a leaf is pure
    or unsplittable (fewer than 2 rows or every feature constant on them: with min_samples_leaf = 1 the draw goes on until it finds a
    feature that is not constant, and a Gini split never has a negative improvement).  Returns the number of leaves."""
    x32 = np.asarray(x32, dtype=np.float32)
    y, weight = np.asarray(y).astype(np.int64), np.asarray(weight).astype(np.int64)
    leaves, seen = 0, 0
    stack = [(0, np.flatnonzero(weight != 0))]
    while stack:
        node, rows = stack.pop()
        seen += 1
        counts = np.bincount(y[rows], weights=weight[rows], minlength=n_classes).astype(np.int64)
        w_node = int(counts.sum())
        assert int(tree["n_node_samples"][node]) == rows.shape[0] and float(tree["weighted_n_node_samples"][node]) == float(w_node), node
        assert np.array_equal(np.asarray(tree["value"][node]), counts.astype(np.float64) / np.float64(w_node)), node
        assert float(tree["impurity"][node]) == float(_gini(counts, w_node)), node
        left, right = int(tree["children_left"][node]), int(tree["children_right"][node])
        if left < 0:
            assert right < 0 and int(tree["feature"][node]) == -2 and float(tree["threshold"][node]) == -2.0, node
            pure = np.count_nonzero(counts) == 1
            splittable = rows.shape[0] >= 2 and bool(np.any(x32[rows].max(0) > x32[rows].min(0)))
            assert pure or not splittable, node
            leaves += 1
            continue
        assert left == node + 1 and right > left, node
        go_left = x32[rows, int(tree["feature"][node])].astype(np.float64) <= float(tree["threshold"][node])
        n_left = int(go_left.sum())
        assert 1 <= n_left < rows.shape[0], node
        assert int(tree["missing_go_to_left"][node]) == int(n_left > rows.shape[0] - n_left), node
        stack.append((right, rows[~go_left]))
        stack.append((left, rows[go_left]))
    assert seen == np.asarray(tree["feature"]).shape[0]
    return leaves


def score_trees(trees, z32):
    """What scikit-learn's forests compute from fitted trees for the float32 rows z32: per tree the leaf each row reaches
    (x <= threshold goes left), the leaves' values summed in tree order and divided by the tree count.  Returns [rows][outputs]."""
    z = np.asarray(z32, dtype=np.float32).astype(np.float64)
    total = np.zeros((z.shape[0], np.asarray(trees[0]["value"]).shape[1]))
    for t in trees:
        feature, threshold = np.asarray(t["feature"]), np.asarray(t["threshold"])
        left, right = np.asarray(t["children_left"]), np.asarray(t["children_right"])
        node = np.zeros(z.shape[0], dtype=np.int64)
        while True:
            inner = np.flatnonzero(left[node] >= 0)
            if not inner.size:
                break
            at = node[inner]
            node[inner] = np.where(z[inner, feature[at]] <= threshold[at], left[at], right[at])
        total += np.asarray(t["value"])[node]
    return total / len(trees)


def expected_chunks(jobs, kind, labels=None):
    """The chunks a sweep must fit these jobs in, as lists of job numbers: the packing rule of lib_treefit.hpp restated.  A job takes
    4 n n_dims bytes of float32 rows, 4 bytes per weight (one per row and tree with a bootstrap, none for extra trees), 40 bytes per
    node of capacity (a stack record and a packed node) and 8 k bytes per node for the values (k: the classes present in the job's
    training rows, 1 for the regressor); a tree's capacity is 2 (in-bag rows) - 1 nodes.  A job joins the current chunk unless it
    is not the chunk's first and the sum would exceed 2^30 bytes.  kind: "randomforest", "extratrees" or "regressor"."""
    chunks, used = [], 0
    for j, (tr, _, mean, _, (n_estimators, seed)) in enumerate(jobs):
        n, n_dims = len(tr), len(mean)
        k = 1 if kind == "regressor" else int(np.unique(np.asarray(labels)[tr]).shape[0])
        if kind == "extratrees":
            weights, nodes = 0, n_estimators * (2 * n - 1)
        else:
            weights = n_estimators * n
            nodes = sum(2 * int(np.count_nonzero(bootstrap_weights(s, n))) - 1 for s in forest_seeds(seed, n_estimators))
        size = 4 * n * n_dims + 4 * weights + 40 * nodes + 8 * k * nodes
        if chunks and used + size <= 2 ** 30:
            chunks[-1].append(j)
            used += size
        else:
            chunks.append([j])
            used = size
    return chunks


CHUNK_TREES = {"randomforest": 64, "extratrees": 40}
CHUNK_LAYOUT = [[0, 1], [2, 3, 4], [5, 6]]                 # what expected_chunks gives for chunk_sweep_case, either kind
CHUNK_TINY, CHUNK_NO_TEST = 3, 5


def _chunk_stats(j, Z):
    """A big job's own mean and scale: one column is moved out to -2^(18 + j % 4), where float32 keeps 1/32 .. 1/4 of the 1/64 grid
    the values lie on, so the float32 rows -- and with them the trees -- are those of THIS job's statistics and of no other's."""
    mean, scale = Z.mean(0), Z.std(0) * (1.0 + j / 8.0)
    mean[j % 3] = -float(2 ** (18 + j % 4))
    return mean, scale


def chunk_sweep_case(kind):
    """A classifier sweep that needs three chunks of the real 1 GiB bound: the wide_limit_case rows plus 400 rows for the test lists;
    seven jobs big, big, big, tiny, big, big, big.  A big job trains on its own permutation of the 8192 rows (64 classes) with its
    own mean, scale and seed and has 50 test rows (job 5: none); the tiny job trains 3 trees on 5 rows of the classes 17 and 40 and
    has 7 test rows.  Returns (X, y, jobs) with jobs of (train_idx, test_idx, mean, scale, (n_estimators, seed))."""
    c = wide_limit_case()
    rs = np.random.RandomState(606)
    y2 = rs.randint(0, 64, 400)
    X2 = np.round(np.stack([y2 % 8 + 0.4 * rs.randn(400), y2 // 8 + 0.4 * rs.randn(400), rs.randn(400)], axis=1) * 64) / 64
    X, y = np.concatenate([c["X"], X2]), np.concatenate([c["y"], y2]).astype(np.float64)
    n, jobs = c["X"].shape[0], []
    for j in range(7):
        seed = int(rs.randint(np.iinfo(np.int32).max))
        if j == CHUNK_TINY:
            tr = np.concatenate([np.flatnonzero(c["y"] == 17)[:3], np.flatnonzero(c["y"] == 40)[:2]])
            jobs.append((tr, n + rs.permutation(400)[:7], np.zeros(3), np.ones(3), (3, seed)))
            continue
        tr = rs.permutation(n)
        te = n + rs.permutation(400)[:0 if j == CHUNK_NO_TEST else 50]
        jobs.append((tr, te) + _chunk_stats(j, X[tr]) + ((CHUNK_TREES[kind], seed),))
    return X, y, jobs


def job_tasks(y, job, bootstrap, forest_tree_seeds, tree_inputs):
    """One job of a sweep as the tasks tree_fit / tree_fit_regression take: per tree the seed and the weights that
    train_forest_device derives, through the two functions of audioTrainTest handed in."""
    tr, _, mean, scale, (n_estimators, seed) = job
    rows, labels = np.asarray(tr), np.asarray(y)[tr]
    return [(rows, labels) + tree_inputs(s, rows.shape[0], bootstrap)[::-1] + (mean, scale) for s in forest_tree_seeds(seed, n_estimators)]
