"""A plain NumPy restatement of the gradient-boosting fit that paa_boost_fit_splits_f64 runs on the device (csrc/kernels_boost.hpp, the
kFriedman instance of tree_fit_kernel in csrc/kernels_treefit.hpp, csrc/lib_boost.hpp): scikit-learn 1.7.2's
GradientBoostingClassifier(n_estimators) with its defaults -- log-loss, learning_rate 0.1, subsample 1, init = the class priors, per
stage one DecisionTreeRegressor(criterion="friedman_mse", max_depth=3) per class (one for two classes) on the negative gradients,
then one Newton step per leaf (_update_terminal_regions).  Written from scikit-learn's behaviour, not for speed.

The tree is treefit_reg_ref's (draws, constant-feature bookkeeping, candidates, thresholds, preorder ids) with
 * FriedmanMSE over MSE: node and children impurity are MSE's; the proxy is diff diff / (w_left w_right) with
   diff = w_right sum_left - w_left sum_right; the improvement is diff diff / (w_left w_right weighted_n_node_samples);
 * a node is also a leaf when depth >= max_depth (the root has depth 0);
 * THE DEVICE'S SUMMATION ORDER (dev_sum, dev_prefix): a list is cut into 256 consecutive chunks of ceil(n / 256) values, chunk t is
   added serially from 0.0, the 256 partial sums by a xor butterfly within each group of 64 (offsets 32 .. 1) and the four group
   sums as ((s0 + s1) + s2) + s3; the prefix left of a candidate is (the earlier groups' totals, in order from 0.0) + (the
   Hillis-Steele scan value of the chunk before, offsets 1 .. 32) and from there serial within the chunk.  The sorted order is by
   (value, weight, the row's place).
scikit-learn's own order (its introsort, in-place partition and NumPy's pairwise sums) is not restated: where every sum is exact in
FP64 the order is immaterial and the three agree bit for bit -- stage 0 of balanced jobs with 2, 4 or 8 classes (residuals 1/K - y)
and the builder's cases with targets in eighths; elsewhere they agree to the last places, and check_boost_stage holds a tree to what
CART demands in exact arithmetic."""
from fractions import Fraction

import numpy as np

import treefit_ref as T
import treefit_reg_ref as RR
from treefit_ref import EPS, RAND_R_MAX, THR32, FixedSeed, standardize32  # noqa: F401

FIELDS = RR.FIELDS
LEARNING_RATE, MAX_DEPTH = 0.1, 3
U = Fraction(1, 2 ** 52)
_LANES = np.arange(64)


def dev_sum(v):
    """The sum of v in the device's order."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[0]
    chunk = max((n + 255) // 256, 1)
    pad = np.zeros(256 * chunk)
    pad[:n] = v
    part = np.cumsum(np.concatenate([np.zeros((256, 1)), pad.reshape(256, chunk)], axis=1), axis=1)[:, -1].reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, _LANES ^ o]
    s = part[:, 0]
    return np.float64(((s[0] + s[1]) + s[2]) + s[3])


def dev_prefix(v):
    """Per position p the sum of v[:p] in the device's order (the candidate scan)."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[0]
    chunk = max((n + 255) // 256, 1)
    pad = np.zeros(256 * chunk)
    pad[:n] = v
    rows = pad.reshape(256, chunk)
    inc = np.cumsum(np.concatenate([np.zeros((256, 1)), rows], axis=1), axis=1)[:, -1].reshape(4, 64)
    for o in (1, 2, 4, 8, 16, 32):
        shifted = np.concatenate([np.zeros((4, o)), inc[:, :-o]], axis=1)
        inc = np.where(_LANES >= o, shifted + inc, inc)
    base, run = np.zeros(4), np.float64(0.0)
    for w in range(4):
        base[w] = run
        run = run + inc[w, 63]
    before = np.concatenate([np.zeros((4, 1)), inc[:, :-1]], axis=1)
    ev = (base[:, None] + before).reshape(256)
    walk = np.cumsum(np.concatenate([ev[:, None], rows], axis=1), axis=1)[:, :-1]
    return walk.reshape(-1)[:n]


def _impurity(sq, s, w):
    return sq / w - (s / w) * (s / w)


def fit_tree(x32, y, weight, seed, max_depth):
    """One tree of a boosting stage over the rows of x32 [n][n_dims] (float32) with targets y, integer weights and the rand_r seed.
    Returns a dict of scikit-learn's tree_ arrays (value as [nodes][1]) and "rows": per node the rows it holds, in node order."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.float64)
    weight = np.asarray(weight).astype(np.int64)
    n_dims = x32.shape[1]
    rng = T._Rand(seed)
    features = list(range(n_dims))
    constant = [0] * n_dims
    samples = np.flatnonzero(weight != 0)
    out = {k: [] for k in FIELDS}
    node_rows = []
    stack = [(samples, -1, False, None, 0, 0)]
    while stack:
        rows, parent, is_left, impurity, n_known, depth = stack.pop()
        n = rows.shape[0]
        wf = weight[rows].astype(np.float64)
        wy = wf * y[rows]
        sum_total, sq_total, w_node = dev_sum(wy), dev_sum(wy * y[rows]), np.float64(weight[rows].sum())
        if impurity is None:
            impurity = _impurity(sq_total, sum_total, w_node)
        is_leaf = n < 2 or depth >= max_depth or impurity <= EPS
        best = None
        if not is_leaf:
            best_proxy = -np.inf
            f_i, n_found, n_drawn, n_total, n_visited = n_dims, 0, 0, n_known, 0
            while f_i > n_total and (n_visited < n_dims or n_visited <= n_found + n_drawn):
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
                order = np.lexsort((rows, weight[rows], v))
                sv = v[order]
                sl = dev_prefix(wy[order])[1:]                  # left of position p = 1 .. n - 1
                wl = np.cumsum(wf[order])[:-1]
                sr, wr = sum_total - sl, w_node - wl
                diff = wr * sl - wl * sr
                proxy = diff * diff / (wl * wr)
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
                # (the device adds the left rows inside the NODE's chunks: the right rows count as 0.0)
                sum_l, sq_l, wl = dev_sum(np.where(go_left, wy, 0.0)), dev_sum(np.where(go_left, wy * y[rows], 0.0)), np.float64(weight[lrows].sum())
                wr, sum_r = w_node - wl, sum_total - sum_l
                imp_l, imp_r = _impurity(sq_l, sum_l, wl), _impurity(sq_total - sq_l, sum_r, wr)
                diff = wr * sum_l - wl * sum_r
                improvement = diff * diff / (wl * wr * w_node)
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
        node_rows.append(rows)
        if not is_leaf:
            stack.append((rrows, node, False, imp_r, n_known, depth + 1))
            stack.append((lrows, node, True, imp_l, n_known, depth + 1))
    res = {k: np.asarray(v) for k, v in out.items()}
    res["value"] = res["value"].reshape(-1, 1).astype(np.float64)
    res["rows"] = node_rows
    return res


def tree_arrays(tree_):
    """The arrays of a fitted scikit-learn Tree as a dict (value [nodes][1])."""
    res = {k: np.asarray(getattr(tree_, k)) for k in T.TREE_FIELDS if k != "value"}
    res["value"] = np.asarray(tree_.value).reshape(tree_.node_count, 1)
    res["missing_go_to_left"] = np.asarray(tree_.missing_go_to_left)
    return res


def sklearn_tree(x32, y, weight, random_state, max_depth):
    """scikit-learn's own tree for the same problem: DecisionTreeRegressor(criterion="friedman_mse", max_depth, random_state)."""
    from sklearn.tree import DecisionTreeRegressor
    m = DecisionTreeRegressor(criterion="friedman_mse", max_depth=max_depth, random_state=random_state)
    m.fit(np.asarray(x32, dtype=np.float32), np.asarray(y, dtype=np.float64), sample_weight=np.asarray(weight, dtype=np.float64))
    return tree_arrays(m.tree_)


def assert_same_tree(a, b, what=""):
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), (what, k)


# ---- the loss -----------------------------------------------------------------------------------------------------------------

def init_raw(y, K):
    """_raw_predict_init of init=None: the class fractions clipped to float32's eps, through the loss's link.  Two classes:
    scipy.special.logit of the second class's fraction; more: log(p / gmean(p)) with scipy.stats.gmean = exp(mean(log p))."""
    prior = np.bincount(np.asarray(y, dtype=np.int64), minlength=K) / len(y)
    eps = np.finfo(np.float32).eps
    p = np.clip(prior, eps, 1 - eps)
    if K == 2:
        from scipy.special import logit
        return np.array([logit(p[1])])
    gm = np.exp(np.mean(np.log(p)))
    return np.log(p / gm)


def _log1pexp(x):
    if x <= -37:
        return np.exp(x)
    if x <= -2:
        return np.log1p(np.exp(x))
    if x <= 18:
        return np.log(1.0 + np.exp(x))
    if x <= 33.3:
        return x + np.exp(-x)
    return x


def gradient_and_loss(raw, y, K):
    """raw [n][k_out], class indices y: (the negative gradients [n][k_out], the mean loss in the device's order -- train_score_ of the
    stage that gave raw)."""
    n = raw.shape[0]
    res, loss = np.zeros_like(raw), np.zeros(n)
    if K == 2:
        for i in range(n):
            z, yd = raw[i, 0], np.float64(y[i])
            loss[i] = _log1pexp(z) - yd * z
            if z > -37:
                e = np.exp(-z)
                res[i, 0] = -(((1.0 - yd) - yd * e) / (1.0 + e))
            else:
                res[i, 0] = -(np.exp(z) - yd)
        return res, np.float64(2.0) * (dev_sum(loss) / np.float64(n))
    for i in range(n):
        top = raw[i, 0]
        for k in range(1, K):
            if top < raw[i, k]:
                top = raw[i, k]
        s = np.float64(0.0)
        for k in range(K):
            s = s + np.exp(raw[i, k] - top)
        loss[i] = (np.log(s) + top) - raw[i, y[i]]
        for k in range(K):
            res[i, k] = -(np.exp(raw[i, k] - top) / s - (1.0 if y[i] == k else 0.0))
    return res, dev_sum(loss) / np.float64(n)


def leaf_value(r, yk, K):
    """The Newton step of one leaf: its rows' residuals r and indicators yk, in node order."""
    n = np.float64(len(r))
    num = dev_sum(r) / n
    num = num * (1.0 if K == 2 else np.float64(K - 1) / np.float64(K))
    p = yk - r
    den = dev_sum(p * (1.0 - p)) / n
    return np.float64(0.0) if abs(den) < 1e-150 else num / den


def fit(x32, y, K, n_stages, seeds, max_depth=MAX_DEPTH, learning_rate=LEARNING_RATE):
    """The whole fit: class indices y in 0 .. K - 1, one rand_r seed per tree (stage-major, then class).  Returns (trees, a list
    stage-major then class, leaf values in place; train_score [n_stages]; raw [n][k_out]; init [k_out])."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.int64)
    n, k_out = x32.shape[0], 1 if K == 2 else K
    init = init_raw(y, K)[:k_out]
    raw = np.tile(init, (n, 1)).astype(np.float64)
    ones = np.ones(n, dtype=np.int64)
    trees, score = [], np.zeros(n_stages)
    for s in range(n_stages):
        res, loss = gradient_and_loss(raw, y, K)
        if s:
            score[s - 1] = loss
        for k in range(k_out):
            cls = 1 if K == 2 else k
            tree = fit_tree(x32, res[:, k], ones, seeds[s * k_out + k], max_depth)
            yk = (y == cls).astype(np.float64)
            for node in np.flatnonzero(tree["children_left"] < 0):
                rows = tree["rows"][node]
                v = leaf_value(res[rows, k], yk[rows], K)
                tree["value"][node, 0] = v
                raw[rows, k] = raw[rows, k] + learning_rate * v
            trees.append(tree)
    score[n_stages - 1] = gradient_and_loss(raw, y, K)[1]
    return trees, score, raw, init


def tree_seeds(random_state, n_trees):
    """The rand_r seeds scikit-learn's trees draw from the ensemble's ONE RandomState: one randint(0, RAND_R_MAX) each, in order."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    return [int(rs.randint(0, RAND_R_MAX)) for _ in range(n_trees)]


def sklearn_fit(x32, y, n_stages, random_state):
    from sklearn.ensemble import GradientBoostingClassifier
    return GradientBoostingClassifier(n_estimators=n_stages, random_state=random_state).fit(np.asarray(x32, dtype=np.float32), y)


def predict_raw(trees, init, k_out, z32, learning_rate=LEARNING_RATE):
    """raw [q][k_out] of rows z32 from trees given as dicts (stage-major, then class): predict_stages' order."""
    z32 = np.asarray(z32, dtype=np.float32)
    raw = np.tile(np.asarray(init, dtype=np.float64), (z32.shape[0], 1))
    for t, tree in enumerate(trees):
        for i in range(z32.shape[0]):
            node = 0
            while tree["children_left"][node] >= 0:
                node = tree["children_left"][node] if np.float64(z32[i, tree["feature"][node]]) <= tree["threshold"][node] else tree["children_right"][node]
            raw[i, t % k_out] = raw[i, t % k_out] + learning_rate * np.asarray(tree["value"]).reshape(-1)[node]
    return raw


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def builder_cases():
    """Builder alone, exact targets (multiples of 1/8 within +-1024): name -> dict(X, y, w, mean, scale, seed, max_depth)."""
    rs = np.random.RandomState(2024)
    out = {}

    def add(name, X, y, depth=3, standardize=False):
        X = np.asarray(X, dtype=np.float64)
        n, d = X.shape
        y = np.asarray(y, dtype=np.float64)
        w = np.ones(n, dtype=np.int32)
        RR.assert_exact(y, w)
        mean, scale = (X.mean(0), np.where(X.std(0) > 0, X.std(0), 1.0)) if standardize else (np.zeros(d), np.ones(d))
        out[name] = dict(X=X, y=y, w=w, mean=mean, scale=scale, seed=int(rs.randint(0, RAND_R_MAX)), max_depth=depth)

    def wave(n, d):
        X = rs.randn(n, d)
        return X, RR.eighths(3.0 * X[:, 0] - 2.0 * np.abs(X[:, d - 1]) + rs.randn(n))

    add("one_row", rs.randn(1, 3), [1.5])
    add("two_rows_equal", [[0.0, 1.0], [1.0, 1.0]], [2.5, 2.5])
    add("two_rows_distinct", [[0.0, 1.0], [1.0, 1.0]], [1.0, -3.125])
    add("constant_target", rs.randn(20, 4), np.full(20, 7.375))
    add("all_constant", np.ones((12, 5)) * [1.0, -2.0, 0.0, 3.5, 1e-9], np.arange(12) / 8)
    add("integer_ties", rs.randint(0, 4, (200, 6)), RR.eighths(rs.randn(200) * 3))
    X = np.zeros((40, 3))
    X[:, 0] = np.float32(0.1) + 5e-8 * np.arange(40) + (np.arange(40) >= 20) * 0.1
    X[:, 1] = np.float32(0.3) + 5e-8 * (np.arange(40) % 7)
    X[:, 2] = np.arange(40) % 3
    add("adjacent_float32_values", X, RR.eighths(rs.randn(40) * 5 + (np.arange(40) % 5) * 3))
    X, y = wave(80, 1)
    add("dims_1", X, y, standardize=True)
    X, y = wave(12, 256)
    add("dims_256", np.round(X * 512) / 512, y)
    for depth in (1, 2, 3, 12):
        X, y = wave(90, 4)
        add("depth_%d" % depth, X, y, depth=depth)
    X = rs.randn(16, 2)
    add("impure_at_the_limit", X, RR.eighths(np.arange(16) * 1.5), depth=2)         # 16 distinct targets, 4 leaves: every leaf impure
    for n in (63, 64, 65, 257, 513):
        X, y = wave(n, 4)
        add("rows_%d" % n, X, y, standardize=True)
    return out


def limit_case(n=8192):
    """The row limit, which is the LDS peak: 8192 rows x 3 dims of coarse float32 values, targets of a few levels, depth 3."""
    rs = np.random.RandomState(98)
    X = np.round(rs.randn(n, 3) * 16).astype(np.float64) / 8
    y = RR.eighths(np.round(2.0 * X[:, 0] - X[:, 2] + rs.randn(n) * 0.5) * 4)
    return dict(X=X, y=y, w=np.ones(n, dtype=np.int32), mean=np.zeros(3), scale=np.ones(3), seed=20250301, max_depth=3)


def gaussian_cases():
    """Builder alone, Gaussian targets: (300 x 9) and (257 x 4: two rows per thread in one chunk)."""
    out = {}
    for name, n, d, seed in (("gauss_300x9", 300, 9, 5), ("gauss_257x4", 257, 4, 6)):
        rs = np.random.RandomState(seed)
        X = rs.randn(n, d)
        out[name] = dict(X=X, y=2.0 * X[:, 0] - X[:, 1] * X[:, 2] + rs.randn(n), w=np.ones(n, dtype=np.int32), mean=np.zeros(d),
                         scale=np.ones(d), seed=int(rs.randint(0, RAND_R_MAX)), max_depth=3)
    return out


def _classes_case(seed, n, d, K, balanced, ties=False):
    rs = np.random.RandomState(seed)
    y = np.arange(n) % K if balanced else np.sort(rs.choice(K, n, p=np.arange(1, K + 1) / np.arange(1, K + 1).sum()))
    y = y[rs.permutation(n)]
    X = rs.randn(n, d) + 0.9 * np.eye(K, d)[y] * 2.0
    X = (np.round(X * 2) / 2 if ties else X).astype(np.float32).astype(np.float64)       # features are float32 values
    return X, y.astype(np.int64)


STAGE0 = {"stage0_2x200x7_ties": (11, 200, 7, 2, True), "stage0_4x120x5": (12, 120, 5, 4, False), "stage0_8x160x6": (13, 160, 6, 8, False)}
WHOLE = {"fit_2x150x5": (21, 150, 5, 2, True, 10), "fit_3x150x9_unbalanced": (22, 150, 9, 3, False, 10), "fit_8x240x12": (23, 240, 12, 8, True, 5)}


HELD_OUT = 24


def stage0_case(name):
    """A balanced job whose stage 0 is exact: (X, y, K, random_state); every row trains."""
    seed, n, d, K, ties = STAGE0[name]
    X, y = _classes_case(seed, n, d, K, True, ties)
    return X, y, K, 1000 + seed


def whole_case(name):
    """(X, y, training rows, held-out rows, K, n_stages, random_state): continuous Gaussian features rounded to float32; the n rows of
    the case train, HELD_OUT further rows of the same kind are held out."""
    seed, n, d, K, balanced, stages = WHOLE[name]
    X, y = _classes_case(seed, n, d, K, balanced)
    X2, y2 = _classes_case(seed + 100, HELD_OUT, d, K, True)
    return np.concatenate([X, X2]), np.concatenate([y, y2]), np.arange(n), n + np.arange(HELD_OUT), K, stages, 2000 + seed


# ---- exact-arithmetic check of one tree --------------------------------------------------------------------------------------------

def check_boost_stage(tree, x32, y, weight, max_depth, y_err=0.0):
    """treefit_reg_ref.check_cart_tree for a stage's tree: walks it with exact arithmetic and asserts what CART with Friedman's proxy
    under a depth limit demands (u = 2^-52; n, W, A = sum w |y| of the node; e = y_err, a bound on the error of every target):
     * n_node_samples and weighted_n_node_samples are exact; value (of an internal node: the mean) is within n u max|y| + e of the
       exact mean; a node at depth max_depth is a leaf and no node lies deeper;
     * an internal node's (feature, threshold) is a candidate of its rows under the midpoint rule, and its exact proxy
       (W sl - wl S)^2 / (wl wr) is within (16 n + 64) W u A^2 + 32 W n e A of the exact maximum over all candidates: a sum of n terms
       errs by at most n (u / 2) A, diff = wr sl - wl sr by 2 W of that, |diff| <= 2 W A and wl wr >= W / 2 give 8 W n u A^2 per proxy
       through the square, the four roundings of products and quotient another 4 u of a proxy <= 8 W A^2; between two proxies twice
       that; targets off by e move a sum by n e, which goes the same way;
     * a leaf above the depth limit is unsplittable or its exact impurity is at most DBL_EPSILON + 4 n u max y^2 + 4 e max|y|.
    Leaf VALUES are not read (the sweep replaces them by Newton steps).  Returns the number of internal nodes."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.float64)
    weight = np.asarray(weight).astype(np.int64)
    yf = [Fraction(float(v)) for v in y]
    e = Fraction(float(y_err))
    n_dims, internal = x32.shape[1], 0
    stack = [(0, np.flatnonzero(weight != 0), 0)]
    seen = 0
    while stack:
        node, rows, depth = stack.pop()
        seen += 1
        n = rows.shape[0]
        W = int(weight[rows].sum())
        S = sum(int(weight[i]) * yf[i] for i in rows)
        Q = sum(int(weight[i]) * yf[i] * yf[i] for i in rows)
        A = sum(int(weight[i]) * abs(yf[i]) for i in rows)
        ymax = max(abs(yf[i]) for i in rows)
        assert depth <= max_depth, node
        assert int(tree["n_node_samples"][node]) == n and float(tree["weighted_n_node_samples"][node]) == float(W), node
        if int(tree["children_left"][node]) < 0:
            assert int(tree["children_right"][node]) < 0 and int(tree["feature"][node]) == -2
            splittable = n >= 2 and depth < max_depth and any(x32[rows, f].max() > x32[rows, f].min() for f in range(n_dims))
            assert not splittable or Q / W - (S / W) ** 2 <= Fraction(EPS) + 4 * n * U * ymax * ymax + 4 * e * ymax, node
            continue
        assert depth < max_depth, node
        assert abs(Fraction(float(np.asarray(tree["value"]).reshape(-1)[node])) - S / W) <= n * U * ymax + e, node
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
                diff = W * sl - wl * S
                proxy = diff * diff / (wl * (W - wl))
                best = proxy if best is None or proxy > best else best
                if g == f and np.float64(sv[p - 1]) <= thr < np.float64(sv[p]):
                    mid = np.float64(sv[p - 1]) / 2.0 + np.float64(sv[p]) / 2.0
                    assert thr == (np.float64(sv[p - 1]) if mid == np.float64(sv[p]) or np.isinf(mid) else mid), node
                    chosen = proxy
        assert chosen is not None, (node, f, thr)                      # a candidate of the node's rows
        assert best - chosen <= (16 * n + 64) * W * U * A * A + 32 * W * n * e * A, (node, float(best - chosen))
        go_left = x32[rows, f].astype(np.float64) <= thr
        assert int(tree["missing_go_to_left"][node]) == int(go_left.sum() > n - go_left.sum())
        stack.append((int(tree["children_right"][node]), rows[~go_left], depth + 1))
        stack.append((int(tree["children_left"][node]), rows[go_left], depth + 1))
    assert seen == len(tree["feature"])
    return internal
