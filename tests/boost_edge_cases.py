"""The inputs of the gradient-boosting edge tests, their references and the margins they rely on, shared by
tests/test_boost_edges_ref_cpu.py (which establishes, without a device, that every frozen case means what it is meant to) and
tests/test_boost_edges_gpu.py (which runs them through boost_gradient_kernel and the kFriedman instance of tree_fit_kernel).
Plain NumPy (and mpmath for the high-precision reference); imports nothing from the package.

(A) jobs with more than one row per thread in the sweep: more than 256 training rows, so that boost_gradient_kernel and the leaf step
    walk chunks of ceil(n / 256) > 1 rows, up to the row limit (8192: chunk 32) and the class limit (64);
(B) saturated and boundary raw predictions, reached through the `init` argument of paa_boost_fit_splits_f64: tiny jobs whose true
    gradients and losses are computed in mpmath, independent of the five ranges of log1pexp and the two of the binomial gradient;
(C) learning rates and depths other than 0.1 and 3, and the builder at kBoostMaxDepth.
The goldens (tests/golden/boost_edges.npz) are made by scripts/make_boost_edges_golden.py from live scikit-learn 1.7.2."""
import hashlib

import numpy as np

import boost_ref as B
import treefit_reg_ref as RR

U = 2.0 ** -52
GRAD_ULPS = 4                           # the project's figure for the gradients (DESIGN K20), here relative to the true value
E_DEVICE = 2                            # ulp assumed for the device's double exp / log / log1p: no document shipped with the toolchain states it
E_HOST = 1                              # glibc's


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------------
# (A) more than one row per thread
# ---------------------------------------------------------------------------------------------------------------------------------
# balanced jobs whose stage 0 is exact (residuals 1/K - y with K a power of two): (seed, rows, dims, classes)
STAGE0 = {"stage0_2x514x4": (31, 514, 4, 2), "stage0_4x1028x3": (32, 1028, 3, 4), "stage0_2x8192x3": (33, 8192, 3, 2),
          "stage0_64x192x6": (34, 192, 6, 64)}
# either side of one row per thread, two classes, one stage, against the restatement: (seed, rows, dims, balanced)
NEAR_256 = {"rows_255": (35, 255, 3, True), "rows_256": (36, 256, 3, True), "rows_257_unbalanced": (37, 257, 3, False)}
# whole fits: (seed, rows, dims, classes, balanced, stages).  A seed is frozen only when two summation orders stay within the gate
# (make_boost_golden.py's rule); 42 for the 777-row case breaks a tie between them and was replaced, as were 45 .. 82 for the
# 63-class case (4 rows per class: ties are common)
WHOLE = {"fit_2x600x5": (41, 600, 5, 2, True, 3), "fit_3x777x4_unbalanced": (43, 777, 4, 3, False, 3), "fit_63x252x5": (83, 252, 5, 63, True, 2)}
# (C) whole fits of one 300-row two-class job under other parameters: name -> (learning_rate, max_depth)
PARAM_CASE = (44, 300, 5, 2, True, 3)
PARAMS = {"lr_1_depth_1": (1.0, 1), "lr_0.5_depth_2": (0.5, 2), "lr_0.1_depth_20": (0.1, 20)}


def stage0_case(name):
    """(X, y, K, random_state); every row trains."""
    seed, n, d, K = STAGE0[name]
    X, y = B._classes_case(seed, n, d, K, True)
    return X, y, K, 1000 + seed


def near_case(name):
    seed, n, d, balanced = NEAR_256[name]
    X, y = B._classes_case(seed, n, d, 2, balanced)
    return X, y, 2, 1000 + seed


def _whole(spec):
    seed, n, d, K, balanced, stages = spec
    X, y = B._classes_case(seed, n, d, K, balanced)
    X2, y2 = B._classes_case(seed + 100, B.HELD_OUT, d, K, True)
    return np.concatenate([X, X2]), np.concatenate([y, y2]), np.arange(n), n + np.arange(B.HELD_OUT), K, stages, 2000 + seed


def whole_case(name):
    """boost_ref.whole_case for the cases of WHOLE: (X, y, training rows, held-out rows, K, n_stages, random_state)."""
    return _whole(WHOLE[name])


def param_case():
    return _whole(PARAM_CASE)


def batch_specs():
    """The batch of the invariance test: (case name, stages) -- one job above 256 rows between two below, with 2, 3 and 1 stages, so that
    n_max is not every job's n and the jobs of stages 1 and 2 are strict prefixes of the chunk."""
    return (("fit_2x150x5", 2), ("fit_3x777x4_unbalanced", 3), ("fit_8x240x12", 1))


def fit_from(x32, y, K, n_stages, seeds, init, max_depth, learning_rate):
    """boost_ref.fit from a GIVEN initial raw score.  Returns (trees, train_score, raw, the residuals of the last stage)."""
    x32 = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.int64)
    n, k_out = x32.shape[0], 1 if K == 2 else K
    raw = np.tile(np.asarray(init, dtype=np.float64)[:k_out], (n, 1))
    ones = np.ones(n, dtype=np.int64)
    trees, score, res = [], np.zeros(n_stages), None
    for s in range(n_stages):
        res, loss = B.gradient_and_loss(raw, y, K)
        if s:
            score[s - 1] = loss
        for k in range(k_out):
            tree = B.fit_tree(x32, res[:, k], ones, seeds[s * k_out + k], max_depth)
            yk = (y == (1 if K == 2 else k)).astype(np.float64)
            for node in np.flatnonzero(tree["children_left"] < 0):
                rows = tree["rows"][node]
                v = B.leaf_value(res[rows, k], yk[rows], K)
                tree["value"][node, 0] = v
                raw[rows, k] = raw[rows, k] + learning_rate * v
            trees.append(tree)
    score[n_stages - 1] = B.gradient_and_loss(raw, y, K)[1]
    return trees, score, raw, res


def row_order_sums():
    """A context in which boost_ref sums in plain row order: the second order of make_boost_golden.py's rule."""
    class _Swap:
        def __enter__(self):
            self.keep = B.dev_sum, B.dev_prefix
            B.dev_sum = lambda v: np.float64(np.cumsum(v)[-1]) if len(v) else np.float64(0.0)
            B.dev_prefix = lambda v: np.concatenate([[0.0], np.cumsum(v)[:-1]])

        def __exit__(self, *exc):
            B.dev_sum, B.dev_prefix = self.keep
    return _Swap()


# ---------------------------------------------------------------------------------------------------------------------------------
# (C) the depth limit binding at kBoostMaxDepth, builder alone
# ---------------------------------------------------------------------------------------------------------------------------------
CHAIN_ROWS = 22


def chain_case(max_depth):
    """22 rows, 22 one-hot columns, 22 distinct targets in eighths: a split can only peel one row, so the tree is a chain.  Under
    max_depth = 20: 41 nodes, depth 20, the last leaf holds 2 rows and is impure; under 21 (what no limit gives): 43 nodes, pure."""
    rs = np.random.RandomState(77)
    y = rs.permutation(CHAIN_ROWS) * 0.625 - 3.0
    RR.assert_exact(y, np.ones(CHAIN_ROWS, dtype=np.int32))
    return dict(X=np.eye(CHAIN_ROWS), y=y, w=np.ones(CHAIN_ROWS, dtype=np.int32), mean=np.zeros(CHAIN_ROWS), scale=np.ones(CHAIN_ROWS),
                seed=4242, max_depth=max_depth)


# ---------------------------------------------------------------------------------------------------------------------------------
# (B) saturated and boundary raw predictions
# ---------------------------------------------------------------------------------------------------------------------------------
def _around(v):
    return (float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf)))


# two classes: 5 rows of class 0 and 3 of class 1; column 0 separates them, column 1 does not
TWO_X = np.array([[-1.0, 0.5], [-1.5, -0.25], [-2.0, 1.0], [-2.5, -1.0], [-3.0, 0.0], [1.0, 0.75], [1.5, -0.5], [2.0, 0.25]])
TWO_Y = np.array([0, 0, 0, 0, 0, 1, 1, 1], dtype=np.int64)
# 0, +-1, +-30, +-40, +-700; the cuts of log1pexp (-37, -2, 18, 33.3), the negatives of 18 and 33.3, each with both neighbours.
# +-745 is left out: the results are denormal and a relative error means nothing.  -720 is the one init below -709.8, where exp(-raw)
# overflows: only there can the binomial gradient's second formula (raw <= -37) be told from the first, whose results agree with it to
# an ulp or two down to -709.  Its class-0 gradients are denormal and are held to their range only (see two_class_truth)
TWO_INITS = ((0.0, 1.0, -1.0, 30.0, -30.0, 40.0, -40.0, 700.0, -700.0) + _around(-2.0) + _around(18.0) + _around(33.3) + _around(-18.0) +
             _around(-33.3) + _around(-37.0) + (-720.0,))
# three classes: 3 rows each; column 0 orders the classes, column 1 sets class 1 apart (the tree of class 1 has one best split)
THREE_X = np.array([[0.0, 0.0], [0.5, 0.25], [1.0, -0.25], [10.0, 5.0], [10.5, 5.5], [11.0, 4.5], [20.0, 0.125], [20.5, -0.125], [21.0, 0.0]])
THREE_Y = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], dtype=np.int64)
# exact 0 and +-1 residuals, ties for the row maximum, a loss of 800.  The third entry: the exact mean loss where it is one, else None
THREE_INITS = (((0.0, -800.0, 800.0), 800.0), ((700.0, -700.0, 0.0), 700.0), ((5.0, 5.0, 5.0), None), ((0.0, 0.0, -1000.0), None),
               ((1e-300, 0.0, -1e-300), None))
THREE_SATURATED = (0, 1)                # every p is 0 or 1 (or 1e-304): every leaf value is 0
EDGE_SEEDS = (101, 202, 303, 404, 505, 606)         # rand_r seeds of a job's trees (two stages x three classes at most)
# landing exactly on a cut: init 0, depth 1, the leaves are -2 and +2, so the raw predictions are -+2 learning_rate to the bit
CUT_RATES = (1.0, 9.0, 16.65, 18.5, 20.0)           # +-2, +-18, +-33.3, +-37, +-40


EDGE_DEPTH, EDGE_RATE = 1, 0.1


def edge_inputs(K):
    return (TWO_X, TWO_Y) if K == 2 else (THREE_X, THREE_Y)


def edge_inits(K):
    """The table as rows of K values (two classes: the one raw score in column 0)."""
    if K == 2:
        return np.array([[v, 0.0] for v in TWO_INITS])
    return np.array([v for v, _ in THREE_INITS])


def edge_fit(K, init, stages):
    """The restatement of one job of the table: depth 1, learning rate 0.1.  (trees, train_score, raw, the last stage's residuals)"""
    X, y = edge_inputs(K)
    return fit_from(X, y, K, stages, EDGE_SEEDS, init, EDGE_DEPTH, EDGE_RATE)


def in_cliff(z, y):
    """Near +-37 p = y - r rounds to 0 or to 2^-53: one ulp of the device's exp can move a leaf value between 0 and 9e15.  For such rows
    only the gradients and finiteness are asserted."""
    return (y == 1 and -39.0 < z < -34.0) or (y == 0 and 34.0 < z < 39.0)


def job_in_cliff(raw, y):
    raw = np.asarray(raw, dtype=np.float64).reshape(len(y), -1)
    return raw.shape[1] == 1 and any(in_cliff(float(raw[i, 0]), int(y[i])) for i in range(len(y)))


# ---- the true gradients and losses ------------------------------------------------------------------------------------------------
PREC = 300                              # bits: beyond what any case needs (every formula below is free of cancellation)


def have_mpmath():
    try:
        import mpmath  # noqa: F401
        return True
    except ImportError:
        return False


class _LongDouble:
    """What the envelope needs of mpmath, in numpy.longdouble: its own roundings (2^-64) are far below the half ulps it counts."""
    mpf = staticmethod(lambda v: np.longdouble(v))
    exp, log, log1p = staticmethod(np.exp), staticmethod(np.log), staticmethod(np.log1p)
    fsum = staticmethod(lambda it: sum(list(it), np.longdouble(0)))
    ldexp = staticmethod(lambda m, e: np.ldexp(np.longdouble(m), e))


def _mp():
    if not have_mpmath():
        assert np.finfo(np.longdouble).nmant >= 63
        return _LongDouble
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.prec = PREC
    return ctx


def mp_two(z, y):
    """(y - sigmoid(z), log(1 + e^z) - y z) of one row as mpf, free of cancellation: 1 - sigmoid(z) = sigmoid(-z), and
    log(1 + e^z) - z = log1p(e^-z).  log1p, not log(1 + .): the naive form is 0 at z = -700 at any fixed precision."""
    mp = _mp()
    z = mp.mpf(float(z))
    if y:
        return 1 / (1 + mp.exp(z)), mp.log1p(mp.exp(-z))
    return -1 / (1 + mp.exp(-z)), mp.log1p(mp.exp(z))


def mp_multi(raw, y):
    """((y == k) - softmax(raw)[k] for every k, -log softmax(raw)[y]) of one row as mpf: 1 - p_y = (the others' sum) / sum, and the
    loss is log1p(sum over j != y of e^(raw_j - raw_y))."""
    mp = _mp()
    r = [mp.mpf(float(v)) for v in raw]
    top = max(r)
    e = [mp.exp(v - top) for v in r]
    total = mp.fsum(e)
    grad = [mp.fsum(e[j] for j in range(len(r)) if j != k) / total if k == y else -e[k] / total for k in range(len(r))]
    return grad, mp.log1p(mp.fsum(mp.exp(r[j] - r[y]) for j in range(len(r)) if j != y))


def ld_two(z, y):
    """mp_two in numpy.longdouble (x87: 63 mantissa bits), the fallback where mpmath is missing."""
    L = np.longdouble
    assert np.finfo(L).nmant >= 63
    z = L(z)
    with np.errstate(over="ignore", under="ignore"):
        if y:
            return L(1) / (L(1) + np.exp(z)), _ld_softplus(-z)
        return -L(1) / (L(1) + np.exp(-z)), _ld_softplus(z)


def _ld_softplus(z):
    with np.errstate(over="ignore", under="ignore"):
        return z + np.log1p(np.exp(-z)) if z > 0 else np.log1p(np.exp(z))


def ld_multi(raw, y):
    L = np.longdouble
    assert np.finfo(L).nmant >= 63
    r = np.asarray(raw, dtype=np.float64).astype(L)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(r - r.max())
        total = e.sum()
        grad = [np.delete(e, k).sum() / total if k == y else -e[k] / total for k in range(len(r))]
        d = np.delete(r - r[y], y)
        m = d.max()
        loss = m + np.log(np.exp(r - r[y] - m).sum()) if m > 0 else np.log1p(np.exp(d).sum())
    return grad, loss


def true_rows(raw, y, K, use_mpmath=None):
    """The true negative gradients [n][k_out] and per-row losses [n] of raw predictions raw [n][k_out] (two classes: the loss WITHOUT
    the factor 2), as objects of the high-precision type (mpf, or longdouble when mpmath is missing / use_mpmath is False)."""
    use = have_mpmath() if use_mpmath is None else use_mpmath
    raw = np.asarray(raw, dtype=np.float64).reshape(len(y), -1)
    grads, losses = [], []
    for i in range(len(y)):
        if K == 2:
            g, l = (mp_two if use else ld_two)(raw[i, 0], int(y[i]))
            g = [g]
        else:
            g, l = (mp_multi if use else ld_multi)(raw[i], int(y[i]))
        grads.append(g)
        losses.append(l)
    return grads, losses


TINY = float(np.finfo(np.float64).tiny)


def gradient_ratio(got, truth, own=False):
    """How far a device gradient is from the true one, in units of GRAD_ULPS x 2^-52 x |truth|; 0.0 / inf where equality is demanded
    and holds / fails.  Equality (zeros of either sign are equal) is demanded where the truth rounds to exactly 0 or +-1; a truth
    below the smallest normal number is held to its range alone: the same sign and at most the smallest normal number.
    own: the softmax gradient of a row's OWN class, which scikit-learn's formula forms as 1 - p_y from the rounded p_y.  Where p_y
    rounds to 1 the result is 0 whatever the truth (1e-304 at (700, -700, 0)): the formula itself cancels, and the restatement in
    glibc misses a bound relative to the truth by 2^50 there.  What the kernel rounds is p_y, so the unit is GRAD_ULPS x 2^-52 of
    the larger of |truth| and the true p_y = 1 - truth."""
    t = float(truth)
    got = float(got)
    if not np.isfinite(got):
        return np.inf
    if t == 0.0 or abs(t) == 1.0:
        return 0.0 if got == t else np.inf
    if abs(t) < TINY:
        return 0.0 if abs(got) <= TINY and (got == 0.0 or (got > 0) == (t > 0)) else np.inf
    scale = max(abs(truth), abs(1 - truth)) if own else abs(truth)
    return float(abs(type(truth)(got) - truth) / scale) / (GRAD_ULPS * U)


def worst_gradient_ratio(resid, raw, y, K, use_mpmath=None):
    resid = np.asarray(resid, dtype=np.float64).reshape(len(y), -1)
    grads, _ = true_rows(raw, y, K, use_mpmath)
    return max(gradient_ratio(resid[i, k], grads[i][k], K > 2 and k == int(y[i])) for i in range(len(y)) for k in range(resid.shape[1]))


# ---- the envelope of the loss ------------------------------------------------------------------------------------------------------
class _Iv:
    """A closed interval of mpf."""

    def __init__(self, lo, hi=None):
        self.lo, self.hi = lo, lo if hi is None else hi

    def widen(self, rel, mp):
        """Every point moved by at most rel of itself (and half a denormal spacing)."""
        tiny = mp.ldexp(1, -1075)
        return _Iv(self.lo - abs(self.lo) * rel - tiny, self.hi + abs(self.hi) * rel + tiny)

    def mag(self):
        return max(abs(self.lo), abs(self.hi))


def loss_envelope(raw, y, K, E):
    """[lo, hi] as mpf: every value that scikit-learn's loss formula -- log1pexp(z) - y z in its five ranges and twice the mean for two
    classes, (log(sum_k exp(raw_k - max)) + max) - raw_y for more -- can give in double when every exp, log and log1p result is within
    E ulp of the true one (relative E 2^-52), every other operation rounds by at most half an ulp (relative 2^-53) and the n terms are
    added in any order (n 2^-53 of the sum of |terms|).  The formula cancels for class-1 rows at large z, (z + e^-z) - z, so the
    interval is wide there by the formula's own nature; the TRUE mean loss need not lie in it, a faithful evaluation does."""
    mp = _mp()
    raw = np.asarray(raw, dtype=np.float64).reshape(len(y), -1)
    f, h = mp.mpf(E) * mp.mpf(U), mp.mpf(U) / 2
    n = len(y)
    fn = lambda fun, a: _Iv(fun(a.lo), fun(a.hi)).widen(f, mp)                   # noqa: E731  (a monotone function, E ulp)
    add = lambda a, b: _Iv(a.lo + b.lo, a.hi + b.hi).widen(h, mp)                 # noqa: E731
    sub = lambda a, b: _Iv(a.lo - b.hi, a.hi - b.lo).widen(h, mp)                 # noqa: E731
    terms = []
    for i in range(n):
        if K == 2:
            x, z = float(raw[i, 0]), _Iv(mp.mpf(float(raw[i, 0])))
            if x <= -37.0:
                t = fn(mp.exp, z)
            elif x <= -2.0:
                t = fn(mp.log1p, fn(mp.exp, z))
            elif x <= 18.0:
                t = fn(mp.log, add(_Iv(mp.mpf(1)), fn(mp.exp, z)))
            elif x <= 33.3:
                t = add(z, fn(mp.exp, _Iv(-z.lo)))
            else:
                t = z
            terms.append(sub(t, z) if y[i] else t)                                  # (y z is exact; t - 0 z = t)
        else:
            r = [mp.mpf(float(v)) for v in raw[i]]
            top = max(r)
            total = _Iv(mp.mpf(0))
            for v in r:
                total = add(total, fn(mp.exp, _Iv(v - top).widen(h, mp)))
            terms.append(sub(add(fn(mp.log, total), _Iv(top)), _Iv(r[int(y[i])])))
    order = n * h * mp.fsum(t.mag() for t in terms)
    total = _Iv(mp.fsum(t.lo for t in terms) - order, mp.fsum(t.hi for t in terms) + order)
    mean = _Iv(total.lo / n, total.hi / n).widen(h, mp)
    factor = 2 if K == 2 else 1
    return mean.lo * factor, mean.hi * factor


def true_mean_loss(raw, y, K, use_mpmath=None):
    """train_score_ of raw predictions in exact arithmetic (two classes: with the factor 2)."""
    _, losses = true_rows(raw, y, K, use_mpmath)
    total = losses[0]
    for v in losses[1:]:
        total = total + v
    return total / len(y) * (2 if K == 2 else 1)


def envelope_fraction(got, raw, y, K, E):
    """(the distance of a returned train_score_ from the true mean loss of raw as a fraction of the envelope's reach from that truth,
    whether it lies inside the envelope, its distance from the envelope's middle as a fraction of the half width).  Where the formula
    returns raw itself (raw > 33.3) the envelope is nearly a point beside the truth and the first figure is 1 by construction; the
    third says how much of the envelope a result used."""
    mp = _mp()
    lo, hi = loss_envelope(raw, y, K, E)
    truth = true_mean_loss(raw, y, K)
    reach = max(abs(hi - truth), abs(truth - lo))
    g = mp.mpf(float(got))
    used = float(abs(g - (lo + hi) / 2) / ((hi - lo) / 2))
    return (float(abs(g - truth) / reach) if reach > 0 else (0.0 if g == truth else np.inf)), bool(np.isfinite(got) and lo <= g <= hi), used


# ---- walking a depth-1 tree ------------------------------------------------------------------------------------------------------------
def leaf_rows(tree, x32):
    """node -> the rows of x32 [n][d] (float32) that a tree given as a dict of arrays sends to that leaf, in row order."""
    out = {}
    for i in range(x32.shape[0]):
        node = 0
        while tree["children_left"][node] >= 0:
            node = tree["children_left"][node] if np.float64(x32[i, tree["feature"][node]]) <= tree["threshold"][node] else tree["children_right"][node]
        out.setdefault(int(node), []).append(i)
    return {k: np.array(v) for k, v in out.items()}
