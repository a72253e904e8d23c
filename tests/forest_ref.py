"""NumPy restatement of scikit-learn's tree-ensemble classifiers as the GPU kernels compute them (kernels_forest.hpp): the
rules that RandomForestClassifier / ExtraTreesClassifier predict_proba / predict and GradientBoostingClassifier
_raw_predict / predict / predict_proba follow (scikit-learn 1.4 and later), with no scikit-learn.

  1. x = (feat - mean) / std in FP64, rounded to float32; a split goes left when float64(x32[feature]) <= threshold.
  2. NaN takes the node's missing_go_to_left way (averaged forests); a float32 infinity raises ValueError, and so does a
     NaN for a boosted model (NaN first).
  3. averaged: proba = (0.0 + value_0[leaf_0] + value_1[leaf_1] + ...) / n_trees, the sum in tree order; label = first
     arg-max.
  4. boosted: raw[k] = init[k], then per stage raw[k] = raw[k] + (learning_rate * value[leaf]); two classes: label =
     raw >= 0, proba = (1 - expit, expit); more: label = first arg-max of raw, proba = softmax.

A model is any object with ForestArrays' attributes (pyaudioanalysis_amd.audioTrainTest.ForestArrays).  synthetic_forest
makes seeded random ensembles of given node counts, depths, classes and dims."""
import numpy as np

NAN_MESSAGE = "Input X contains NaN"
INF_MESSAGE = "Input X contains infinity or a value too large for dtype('float32')"


def to_x32(X):
    """Rule 1's input: the float32 cast of the standardised FP64 rows (values beyond FLT_MAX become inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(X, dtype=np.float64).astype(np.float32)


def check_input(X32, boosted):
    """Rule 2's errors, for the whole call."""
    if boosted and np.isnan(X32).any():
        raise ValueError(NAN_MESSAGE + ".")
    if np.isinf(X32).any():
        raise ValueError(INF_MESSAGE + ".")


def invalid_codes(X32, boosted):
    """The kernel's per-row code: -2 NaN under boosting, -1 an infinity, 0 otherwise."""
    nan = np.isnan(X32).any(axis=1) & boosted
    inf = np.isinf(X32).any(axis=1)
    return np.where(nan, -2, np.where(inf, -1, 0))


def apply_tree(model, t, X32):
    """Leaf node (global index) of every row of X32 in tree t (_tree.pyx _apply_dense)."""
    base, end = int(model.node_offsets[t]), int(model.node_offsets[t + 1])
    cl, cr = model.children_left[base:end], model.children_right[base:end]
    feat, thr = model.feature[base:end], model.threshold[base:end]
    miss = model.missing_go_to_left[base:end].astype(bool)
    node = np.zeros(X32.shape[0], dtype=np.int64)
    rows = np.arange(X32.shape[0])
    active = cl[node] != -1
    while active.any():
        r, n = rows[active], node[active]
        x = X32[r, feat[n]]
        left = np.where(np.isnan(x), miss[n], x.astype(np.float64) <= thr[n])
        node[r] = np.where(left, cl[n], cr[n])
        active = cl[node] != -1
    return base + node


def raw_scores(model, X32):
    """Averaged: the tree sums [n][n_classes] (rule 3 before the division); boosted: raw [n][n_outputs] (rule 4)."""
    n_trees = model.node_offsets.shape[0] - 1
    if model.kind == "averaged":
        value = model.value.reshape(model.threshold.shape[0], -1)
        s = np.zeros((X32.shape[0], value.shape[1]))
        for t in range(n_trees):
            s += value[apply_tree(model, t, X32)]
        return s
    K = model.n_outputs
    raw = np.tile(np.asarray(model.init, dtype=np.float64), (X32.shape[0], 1))
    value = model.value.reshape(-1)
    for s in range(n_trees // K):
        for k in range(K):
            step = model.learning_rate * value[apply_tree(model, s * K + k, X32)]
            raw[:, k] = raw[:, k] + step
    return raw


def predict(model, X, check=True):
    """(label indices, proba, raw) of the FP64 standardised rows X [n][n_dims].  check: raise rule 2's ValueError;
    otherwise the rows it would reject get label -1 / -2 (the kernel's codes)."""
    X32 = to_x32(X)
    boosted = model.kind == "boosted"
    if check:
        check_input(X32, boosted)
    raw = raw_scores(model, X32)
    if not boosted:
        proba = raw / float(model.node_offsets.shape[0] - 1)
        labels = np.argmax(proba, axis=1)
    elif raw.shape[1] == 1:
        with np.errstate(over="ignore"):
            e = 1.0 / (1.0 + np.exp(-raw[:, 0]))
        proba = np.stack([1.0 - e, e], axis=1)
        labels = (raw[:, 0] >= 0).astype(np.int64)
    else:
        labels = np.argmax(raw, axis=1)
        z = np.exp(raw - raw.max(axis=1, keepdims=True))
        proba = z / z.sum(axis=1, keepdims=True)
    codes = invalid_codes(X32, boosted)
    labels = np.where(codes != 0, codes, labels).astype(np.int64)
    return labels, proba, raw


# ---------------------------------------------------------------------------------------------------------------------
# seeded models
# ---------------------------------------------------------------------------------------------------------------------
def _random_tree(rng, n_nodes, max_depth, n_dims, width, boosted, f32_thresholds):
    """One tree of n_nodes (odd) nodes, breadth-first numbered (NOT preorder: the host must re-lay it), depth <= max_depth."""
    n_nodes = max(1, n_nodes | 1)
    depth = [0]
    cl, cr = [-1], [-1]
    open_leaves = [0]
    while len(cl) + 2 <= n_nodes and open_leaves:
        j = int(rng.integers(0, len(open_leaves))) if rng.random() < 0.7 else 0
        i = open_leaves[j]
        open_leaves[j] = open_leaves[-1]
        open_leaves.pop()
        if depth[i] >= max_depth:
            continue
        a, b = len(cl), len(cl) + 1
        cl[i], cr[i] = a, b
        cl += [-1, -1]
        cr += [-1, -1]
        depth += [depth[i] + 1, depth[i] + 1]
        open_leaves += [a, b]
    n = len(cl)
    feature = rng.integers(0, n_dims, n)
    thr = rng.standard_normal(n)
    if f32_thresholds:      # a share of float32-representable thresholds: float32 inputs can equal them exactly
        pick = rng.random(n) < 0.5
        thr[pick] = thr[pick].astype(np.float32).astype(np.float64)
    miss = rng.integers(0, 2, n).astype(np.uint8)
    leaf = np.array(cl) == -1
    feature[leaf] = -2                                          # scikit-learn's TREE_UNDEFINED
    thr[leaf] = -2.0
    if boosted:
        value = rng.standard_normal((n, 1))
    else:
        counts = rng.integers(0, 6, (n, width)).astype(np.float64)
        counts[:, 0] += counts.sum(axis=1) == 0
        value = counts / counts.sum(axis=1, keepdims=True)      # fractions, as tree_.value holds them
    return np.array(cl), np.array(cr), feature, thr, miss, value


def chain_tree(depth, n_dims, width, boosted, rng):
    """A chain: node 2 i splits, its left child 2 i + 1 is a leaf, its right child 2 i + 2 goes on (depth splits)."""
    n = 2 * depth + 1
    cl, cr = -np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64)
    for i in range(depth):
        cl[2 * i], cr[2 * i] = 2 * i + 1, 2 * i + 2
    feature = np.where(cl >= 0, rng.integers(0, n_dims, n), -2)
    thr = np.where(cl >= 0, np.linspace(-3.0, 3.0, n), -2.0)          # rising: a row goes right until x <= thr
    miss = rng.integers(0, 2, n).astype(np.uint8)
    if boosted:
        value = rng.standard_normal((n, 1))
    else:
        value = rng.dirichlet(np.ones(width), n)
    return cl, cr, feature, thr, miss, value


def synthetic_forest(kind, n_trees, n_nodes, max_depth, n_classes, n_dims, seed, learning_rate=0.1, chain_depth=0,
                     f32_thresholds=True):
    """A seeded ensemble with no scikit-learn: kind "averaged" (n_trees trees) or "boosted" (n_trees stages, times
    n_outputs trees).  n_nodes: nodes per tree (an int, or a (low, high) range); chain_depth > 0: the first tree is a chain
    of that depth.  Returns a ForestArrays."""
    from pyaudioanalysis_amd.audioTrainTest import ForestArrays
    rng = np.random.default_rng(seed)
    boosted = kind == "boosted"
    n_out = (1 if n_classes == 2 else n_classes) if boosted else 1
    total = n_trees * n_out
    width = 1 if boosted else n_classes
    parts = []
    for t in range(total):
        if t == 0 and chain_depth:
            parts.append(chain_tree(chain_depth, n_dims, width, boosted, rng))
            continue
        size = n_nodes if np.isscalar(n_nodes) else int(rng.integers(n_nodes[0], n_nodes[1] + 1))
        parts.append(_random_tree(rng, int(size), max_depth, n_dims, width, boosted, f32_thresholds))
    offsets = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    cat = [np.concatenate([p[i] for p in parts]) for i in range(6)]
    value = cat[5][:, 0] if boosted else cat[5]
    init = rng.standard_normal(1 if n_classes == 2 else n_classes) if boosted else None
    return ForestArrays(kind, offsets, cat[0], cat[1], cat[2], cat[3], cat[4], value, np.arange(n_classes, dtype=np.float64),
                        n_dims, learning_rate if boosted else 0.0, init)


def tie_rows(model, n, rng, X=None):
    """n rows whose float32 values equal float32-representable thresholds of their split features (exact ties)."""
    thr, feat = model.threshold, model.feature
    ok = (model.children_left != -1) & (thr.astype(np.float32).astype(np.float64) == thr)
    idx = np.flatnonzero(ok)
    X = np.zeros((n, model.n_dims)) if X is None else X.copy()
    for r in range(n):
        for i in rng.choice(idx, min(len(idx), 3 * model.n_dims), replace=False):
            X[r, feat[i]] = thr[i]
    return X


# ---------------------------------------------------------------------------------------------------------------------
# np.longdouble links of the boosted models, and designed inputs for the edge suite (tests/test_forest_edges_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def boosted_proba_ld(raw):
    """Rule 4's probabilities from FP64 raw scores [n][n_outputs], evaluated in np.longdouble."""
    r = np.asarray(raw, dtype=np.longdouble)
    with np.errstate(over="ignore", under="ignore"):
        if r.shape[1] == 1:
            e = 1 / (1 + np.exp(-r[:, 0]))
            return np.stack([1 - e, e], axis=1)
        z = np.exp(r - r.max(axis=1, keepdims=True))
        return z / z.sum(axis=1, keepdims=True)


F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.nextafter(np.float32(0), np.float32(1)))          # the smallest float32 subnormal
BENIGN = -1.0                                                         # left of every boundary threshold below


def _f32_up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _f32_down(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def boundaries():
    """[(name, threshold, missing_go_to_left, FP64 probe values)]: the places where a split decision turns."""
    eq = float(np.float32(0.3))
    a = float(np.float32(1.7))
    b = _f32_up(a)
    sub = float(np.float32(1e-40))
    half_way = 2.0 ** 128 - 2.0 ** 103                                # FLT_MAX + half a float32 ulp: rounds to inf
    return [
        ("equal_f32", eq, 0, [eq, _f32_up(eq), _f32_down(eq)]),
        # the FP64 value is right of the threshold, its float32 rounding left of it -- and the other way round
        ("rounds_down_across", a + 0.25 * (b - a), 1, [a + 0.4 * (b - a), a + 0.6 * (b - a)]),
        ("rounds_up_across", a + 0.75 * (b - a), 0, [a + 0.6 * (b - a), a + 0.4 * (b - a)]),
        ("zero", 0.0, 1, [-0.0, 0.0, F32_TINY, -F32_TINY, 0.4 * F32_TINY, 0.6 * F32_TINY]),
        ("negative_zero_threshold", -0.0, 0, [0.0, -0.0, F32_TINY]),
        ("subnormal", sub, 1, [sub, _f32_up(sub), _f32_down(sub)]),
        ("flt_max", F32_MAX, 0, [F32_MAX, float(np.nextafter(half_way, 0.0)), half_way, -half_way]),
        ("below_flt_max", _f32_down(F32_MAX), 1, [F32_MAX, _f32_down(F32_MAX), -F32_MAX]),
        ("nan_goes_left", 0.5, 1, [np.nan, 1.0]),
        ("nan_goes_right", 0.5, 0, [np.nan, 0.0]),
    ]


def boundary_side(x, thr, miss):
    """True: left.  scikit-learn's rule, rule 1 and 2 above, with NumPy float32 casts."""
    with np.errstate(over="ignore"):
        x32 = np.float64(x).astype(np.float32)
    return bool(miss) if np.isnan(x32) else bool(np.float64(x32) <= thr)


def boundary_rows():
    """(X [n][n_dims] FP64, want_right [n][n_dims] bool): one row per probe, the other features at BENIGN, then one row
    per probe position with every feature at a probe."""
    B = boundaries()
    rows = []
    for f, (_, _, _, probes) in enumerate(B):
        for p in probes:
            r = np.full(len(B), BENIGN)
            r[f] = p
            rows.append(r)
    for j in range(max(len(b[3]) for b in B)):
        rows.append(np.array([b[3][j % len(b[3])] for b in B]))
    X = np.array(rows)
    right = np.array([[not boundary_side(x, B[f][1], B[f][2]) for f, x in enumerate(r)] for r in X])
    return X, right


def boundary_model(kind, n_classes=3, reverse=False):
    """One stump per boundary, feature f = boundary f.  The right leaf of tree t is worth 2^-(t+1) (in the last class of an
    averaged forest, in the raw score of a two-class boosted model, learning rate 1, init 0): the score is the bit mask of
    the trees that went right, and every partial sum is exact."""
    from pyaudioanalysis_amd.audioTrainTest import ForestArrays
    B = boundaries()
    order = list(range(len(B)))[::-1] if reverse else list(range(len(B)))
    n = 3 * len(B)
    cl, cr = -np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64)
    feature, thr = np.full(n, -2, dtype=np.int64), np.full(n, -2.0)
    miss = np.zeros(n, dtype=np.uint8)
    boosted = kind == "boosted"
    value = np.zeros(n) if boosted else np.zeros((n, n_classes))
    for t, f in enumerate(order):
        cl[3 * t], cr[3 * t] = 1, 2
        feature[3 * t], thr[3 * t], miss[3 * t] = f, B[f][1], B[f][2]
        w = 2.0 ** -(t + 1)
        if boosted:
            value[3 * t + 2] = w
        else:
            value[3 * t + 1, 0] = 1.0
            value[3 * t + 2, 0], value[3 * t + 2, n_classes - 1] = 1.0 - w, w
    classes = np.arange(2 if boosted else n_classes, dtype=np.float64)
    return ForestArrays(kind, np.arange(0, n + 1, 3), cl, cr, feature, thr, miss, value, classes, len(B),
                        1.0 if boosted else 0.0, np.zeros(1) if boosted else None), order


def boundary_mask(right, order):
    """The exact score of boundary_model for the decisions `right` [n][n_dims]."""
    return np.array([sum(2.0 ** -(t + 1) for t, f in enumerate(order) if r[f]) for r in right])


def score_model(scores, learning_rate=1.0, init=None):
    """A boosted model of one stage whose raw score for the row x = (i,) is init + learning_rate * scores[i]: per output a
    chain over feature 0 with thresholds i + 0.5.  scores [n_rows][n_outputs]; one output is the two-class model."""
    from pyaudioanalysis_amd.audioTrainTest import ForestArrays
    S = np.atleast_2d(np.asarray(scores, dtype=np.float64))
    n_rows, K = S.shape
    depth = n_rows - 1
    parts = []
    for k in range(K):
        n = 2 * depth + 1
        cl, cr = -np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64)
        feature, thr, value = np.full(n, -2, dtype=np.int64), np.full(n, -2.0), np.zeros(n)
        for i in range(depth):
            cl[2 * i], cr[2 * i], feature[2 * i], thr[2 * i] = 2 * i + 1, 2 * i + 2, 0, i + 0.5
            value[2 * i + 1] = S[i, k]
        value[2 * depth] = S[depth, k]
        parts.append((cl, cr, feature, thr, value))
    offsets = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    cat = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    n_classes = 2 if K == 1 else K
    init = np.zeros(K) if init is None else np.asarray(init, dtype=np.float64)
    return ForestArrays("boosted", offsets, cat[0], cat[1], cat[2], cat[3], np.zeros(offsets[-1], dtype=np.uint8), cat[4],
                        np.arange(n_classes, dtype=np.float64), 1, learning_rate, init)
