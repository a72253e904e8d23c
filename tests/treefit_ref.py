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
