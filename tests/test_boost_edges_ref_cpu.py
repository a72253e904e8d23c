"""What the gradient-boosting edge tests (tests/test_boost_edges_gpu.py) rely on, established without a device on the restatement of
tests/boost_ref.py alone: every frozen case of tests/boost_edge_cases.py is regenerated to its recorded checksum; the restatement
equals the goldens of live scikit-learn 1.7.2 where the sums are exact and is within the 1e-9 gate elsewhere, in the device's
summation order AND in plain row order (no case sits on a tie that two orders break differently); the two high-precision references
(mpmath at 300 bits, numpy.longdouble) agree on every case; the glibc restatement is within 4 x 2^-52 of the true gradients, relative,
and inside the loss envelope at 1 ulp; the exact leaf values the device is held to are the restatement's; and no case outside the
declared cliff bands has a row in one.  No GPU needed."""
import numpy as np
import pytest

import boost_edge_cases as E
import boost_ref as B
from test_boost_cpu import FIELDS, GATE, golden, live_sklearn, rel, same_tree

needs_mpmath = pytest.mark.skipif(not E.have_mpmath(), reason="mpmath is not installed: the tests fall back to numpy.longdouble")


def edges_golden():
    g = golden("boost_edges.npz")
    assert list(g["stage0_names"]) == list(E.STAGE0) and list(g["whole_names"]) == list(E.WHOLE) and list(g["param_names"]) == list(E.PARAMS)
    assert g["cut_rates"].tolist() == list(E.CUT_RATES)
    return g


def stage0_golden(name):
    g = edges_golden()
    p = "s%d_" % list(E.STAGE0).index(name)
    X, y, K, rs = E.stage0_case(name)
    assert str(g[p + "digest"]) == E.digest(X.astype(np.float32), y) and (int(g[p + "K"]), int(g[p + "random_state"])) == (K, rs)
    return g, p, X, y, K, rs


def whole_golden(name):
    """test_boost_cpu.whole_golden for the cases of boost_edge_cases.WHOLE and PARAMS (a PARAMS name: the 300-row job)."""
    g = edges_golden()
    if name in E.WHOLE:
        p, case = "w%d_" % list(E.WHOLE).index(name), E.whole_case(name)
    else:
        p, case = "p%d_" % list(E.PARAMS).index(name), E.param_case()
    X, y, tr, te, K, stages, rs = case
    assert str(g[p + "digest"]) == E.digest(X.astype(np.float32), y)
    assert (int(g[p + "K"]), int(g[p + "n_stages"]), int(g[p + "random_state"])) == (K, stages, rs)
    return g, p, X, y, tr, te, K, stages, rs


def case_params(name):
    return E.PARAMS.get(name, (B.LEARNING_RATE, B.MAX_DEPTH))


@pytest.mark.parametrize("name", list(E.STAGE0))
def test_stage_0_above_256_rows_restatement_equals_the_goldens(name):
    g, p, X, y, K, rs = stage0_golden(name)
    k_out = 1 if K == 2 else K
    assert X.shape[0] > 256 or K == 64
    assert B.tree_seeds(rs, k_out) == g[p + "seeds"].tolist()
    trees, score, raw, init = B.fit(X, y, K, 1, g[p + "seeds"].tolist())
    assert np.array_equal(init, g[p + "init"]) and np.array_equal(raw, g[p + "train_raw"]) and rel(score, g[p + "train_score"]) <= GATE
    for t, tree in enumerate(trees):
        lo, hi = int(g[p + "node_offsets"][t]), int(g[p + "node_offsets"][t + 1])
        for f in FIELDS:
            want = g[p + f][lo:hi]
            assert np.asarray(tree[f]).reshape(-1).astype(want.dtype).tobytes() == want.tobytes(), (name, t, f)
    # the leaf step has more than one row per thread where a leaf holds more than 256 rows: at the row limit, and in the 4-class job
    largest = max(int(g[p + "n_node_samples"][i]) for i in np.flatnonzero(g[p + "children_left"] < 0))
    assert largest > 256 or name in ("stage0_2x514x4", "stage0_64x192x6"), (name, largest)


def near_fits(name):
    X, y, K, rs = E.near_case(name)
    seeds = B.tree_seeds(rs, 2)
    a = B.fit(X, y, K, 2, seeds)
    with E.row_order_sums():
        b = B.fit(X, y, K, 2, seeds)
    return X, y, K, rs, seeds, a, b


@pytest.mark.parametrize("name", list(E.NEAR_256))
def test_rows_near_256_are_free_of_ties(name):
    """Two stages in two summation orders: the same structures, values within the gate; live scikit-learn agrees."""
    X, y, K, rs, seeds, a, b = near_fits(name)
    assert X.shape[0] == int(name.split("_")[1])
    for ta, tb in zip(a[0], b[0]):
        for f in ("children_left", "children_right", "feature", "threshold", "n_node_samples"):
            assert np.array_equal(ta[f], tb[f]), (name, f)
    assert rel(a[1], b[1]) <= GATE and rel(a[2], b[2]) <= GATE
    counts = np.bincount(y)
    assert (counts[0] == counts[1]) == (name == "rows_256") and (name != "rows_257_unbalanced" or abs(int(counts[0]) - int(counts[1])) > 20)
    if name == "rows_256":
        assert a[3][0] == 0.0                                           # the init is exactly 0: stage 0 is exact
    live_sklearn()
    m = B.sklearn_fit(X, y, 2, rs)
    assert rel(a[1], m.train_score_) <= GATE and rel(a[2], m._raw_predict(X.astype(np.float32))) <= GATE
    assert [t["feature"].shape[0] for t in a[0]] == [e.tree_.node_count for e in m.estimators_.ravel()]


@pytest.mark.parametrize("name", list(E.WHOLE) + list(E.PARAMS))
def test_whole_fit_restatement_is_within_the_gate_in_two_orders(name):
    g, p, X, y, tr, te, K, stages, rs = whole_golden(name)
    rate, depth = case_params(name)
    assert (float(g[p + "learning_rate"]), int(g[p + "max_depth"])) == (rate, depth)
    seeds = g[p + "seeds"].tolist()
    assert B.tree_seeds(rs, stages * (1 if K == 2 else K)) == seeds
    trees, score, raw, init = B.fit(X[tr], y[tr], K, stages, seeds, depth, rate)
    with E.row_order_sums():
        trees2, score2, raw2, _ = B.fit(X[tr], y[tr], K, stages, seeds, depth, rate)
    assert np.array_equal(init, g[p + "init"])
    for s, r, t in ((score, raw, trees), (score2, raw2, trees2)):
        assert rel(s, g[p + "train_score"]) <= GATE and rel(r, g[p + "train_raw"]) <= GATE
        assert [tree["feature"].shape[0] for tree in t] == g[p + "node_count"].tolist()
    if depth == 20:                                                     # every tree grew until its leaves were pure, far below the limit of nodes
        for tree in trees:
            leaves = tree["children_left"] < 0                          # (a single row's impurity is the rounding of sq / w - mean^2)
            assert np.all((tree["impurity"][leaves] <= B.EPS) | (tree["n_node_samples"][leaves] == 1)) and tree["feature"].shape[0] > 15


def test_whole_goldens_against_live_scikit_learn():
    live_sklearn()
    from sklearn.ensemble import GradientBoostingClassifier
    for name in list(E.WHOLE) + list(E.PARAMS):
        g, p, X, y, tr, te, K, stages, rs = whole_golden(name)
        rate, depth = case_params(name)
        m = GradientBoostingClassifier(n_estimators=stages, random_state=rs, learning_rate=rate, max_depth=depth).fit(X[tr].astype(np.float32), y[tr])
        assert np.array_equal(m.train_score_, g[p + "train_score"]) and np.array_equal(m.predict_proba(X[te].astype(np.float32)), g[p + "test_proba"])
    for i, rate in enumerate(E.CUT_RATES):
        m = GradientBoostingClassifier(n_estimators=1, learning_rate=rate, max_depth=1, init="zero", random_state=0).fit(E.TWO_X.astype(np.float32), E.TWO_Y)
        assert np.array_equal(m.train_score_, edges_golden()["l%d_train_score" % i])


def test_the_chain_binds_the_depth_limit_at_20():
    g = edges_golden()
    for depth, nodes in ((20, 41), (21, 43)):
        c = E.chain_case(depth)
        assert str(g["chain%d_digest" % depth]) == E.digest(c["X"], c["y"], c["w"], c["mean"], c["scale"])
        tree = B.fit_tree(c["X"].astype(np.float32), c["y"], c["w"], c["seed"], depth)
        same_tree(tree, g, "chain%d_" % depth, depth)
        leaves = tree["children_left"] < 0
        assert tree["feature"].shape[0] == nodes and not leaves[:depth].any() and leaves[depth]          # node d lies at depth d
        assert int(tree["n_node_samples"][depth]) == (2 if depth == 20 else 1)
        assert (tree["impurity"][leaves] > 0).sum() == (1 if depth == 20 else 0) and (depth == 21 or tree["impurity"][20] > 0.05)


# ---- saturated and boundary raw predictions ------------------------------------------------------------------------------------------

def table_jobs(K):
    """(init row, stages) of every job of a table, the 1-stage jobs first."""
    inits = E.edge_inits(K)
    return [(inits[i], s) for s in (1, 2) for i in range(len(inits))]


def test_the_tables_hold_what_the_issue_lists():
    two = list(E.TWO_INITS)
    for v in (0.0, 1.0, -1.0, 30.0, -30.0, 40.0, -40.0, 700.0, -700.0):
        assert v in two
    for v in (-2.0, 18.0, 33.3, -18.0, -33.3, -37.0):
        for w in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
            assert float(w) in two
    assert 745.0 not in two and -745.0 not in two and len(set(two)) == len(two) == 28
    assert np.bincount(E.TWO_Y).tolist() == [5, 3] and np.bincount(E.THREE_Y).tolist() == [3, 3, 3]
    assert E.TWO_X[E.TWO_Y == 0, 0].max() < E.TWO_X[E.TWO_Y == 1, 0].min()
    assert [v for v, _ in E.THREE_INITS] == [(0.0, -800.0, 800.0), (700.0, -700.0, 0.0), (5.0, 5.0, 5.0), (0.0, 0.0, -1000.0), (1e-300, 0.0, -1e-300)]
    # the cliff bands hold -37 and its neighbours and nothing else; no later stage of any job walks into one
    for init, stages in table_jobs(2):
        declared = -39.0 < init[0] < -34.0
        assert E.job_in_cliff(np.full((8, 1), init[0]), E.TWO_Y) == declared == (init[0] in E._around(-37.0))
        if not declared:
            raw = E.edge_fit(2, init, 1)[2]
            assert not E.job_in_cliff(raw, E.TWO_Y), init


@needs_mpmath
@pytest.mark.parametrize("K", (2, 3))
def test_the_two_references_agree(K):
    """mpmath at 300 bits and numpy.longdouble, on the raw predictions every job of the table meets: its init and what stage 0 leaves.
    Gradients to 2^-60 relative and losses to 2^-60 of the larger of the loss and |raw|, the scale of longdouble's own roundings."""
    X, y = E.edge_inputs(K)
    for init in E.edge_inits(K):
        k_out = 1 if K == 2 else K
        for raw in (np.tile(init[:k_out], (len(y), 1)), E.edge_fit(K, init, 1)[2]):
            gm, lm = E.true_rows(raw, y, K, True)
            gl, ll = E.true_rows(raw, y, K, False)
            for i in range(len(y)):
                scale = max(abs(float(lm[i])), float(np.max(np.abs(raw[i]))))
                assert abs(float(lm[i]) - float(ll[i])) <= 2.0 ** -60 * scale + 2.0 ** -1074, (init, i)
                for k in range(k_out):
                    a, b = float(gm[i][k]), float(gl[i][k])
                    assert abs(a - b) <= 2.0 ** -52 * abs(a) / 2 + 2.0 ** -1074, (init, i, k)
                    if abs(a) >= E.TINY:
                        assert abs(float((gm[i][k] - E._mp().mpf(b)) / gm[i][k])) <= 2.0 ** -52, (init, i, k)


@pytest.mark.parametrize("K", (2, 3))
def test_the_restatement_on_the_tables(K):
    """glibc's gradients within the bound of the true ones (the issue's figure for two classes: below 1 x 2^-52), its losses inside the
    envelope at 1 ulp, and the leaf values the device is held to."""
    X, y = E.edge_inputs(K)
    k_out = 1 if K == 2 else K
    worst, worst_fraction = 0.0, 0.0
    for init, stages in table_jobs(K):
        trees, score, raw, resid = E.edge_fit(K, init, stages)
        before = np.tile(init[:k_out], (len(y), 1)) if stages == 1 else E.edge_fit(K, init, 1)[2]
        ratio = E.worst_gradient_ratio(resid, before, y, K)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (init, stages, ratio)
        assert np.all(np.isfinite(raw)) and np.all(np.isfinite(score)) and np.all(np.isfinite(resid))
        if E.job_in_cliff(np.tile(init[:k_out], (len(y), 1)), y):
            continue
        fraction, inside, used = E.envelope_fraction(score[-1], raw, y, K, E.E_HOST)
        worst_fraction = max(worst_fraction, fraction)
        assert inside, (init, stages, fraction)
        if stages == 1:                                                   # two leaves, pure in the tree's class
            for k, tree in enumerate(trees):
                assert tree["feature"].shape[0] == 3
                cls = 1 if K == 2 else k
                for node in (1, 2):
                    assert len(set((y[tree["rows"][node]] == cls).tolist())) == 1, (init, k)
    print("K = %d: the restatement's gradients within %.3f of the bound (%.2f x 2^-52 relative), losses within %.3f of the envelope at %d ulp"
          % (K, worst, worst * E.GRAD_ULPS, worst_fraction, E.E_HOST))
    if K == 2:
        assert worst * E.GRAD_ULPS < 1.0


def test_exact_leaf_values_of_the_restatement():
    """What the issue lists for pure leaves: den exactly 0 on the saturated side, -1 and 0 at -40, -+2 at 0, 50.0 at 40."""
    def leaves(init):
        trees, score, raw, _ = E.edge_fit(2, np.array([init, 0.0]), 1)
        t = trees[0]
        l0, l1 = [int(n) for n in (1, 2)]
        assert set(E.TWO_Y[t["rows"][l0]].tolist()) == {0} and set(E.TWO_Y[t["rows"][l1]].tolist()) == {1}
        return float(t["value"][l0, 0]), float(t["value"][l1, 0]), score, raw
    assert leaves(0.0)[:2] == (-2.0, 2.0)
    v0, v1, score, raw = leaves(40.0)
    assert (v0, v1) == (0.0, 0.0) and np.all(raw == 40.0) and score[0] == 50.0
    assert leaves(-40.0)[:2] == (-1.0, 0.0)
    for init in (700.0, 40.0):
        assert leaves(init)[1] == 0.0 and leaves(-init)[1] == 0.0
    assert leaves(700.0)[0] == 0.0                                     # (class 0 at 700: p = 1 exactly)
    for i in E.THREE_SATURATED:
        init, loss = E.THREE_INITS[i]
        trees, score, raw, _ = E.edge_fit(3, np.array(init), 1)
        assert all(np.all(t["value"][t["children_left"] < 0] == 0.0) for t in trees) and score[0] == loss and np.array_equal(raw, np.tile(init, (9, 1)))
    # the cliff: one ulp of the raw prediction moves the class-1 leaf between 9e15 and 0
    at, above = leaves(-37.0)[1], leaves(float(np.nextafter(-37.0, np.inf)))[1]
    assert at > 1e15 and above == 0.0


def test_landing_on_the_cuts():
    """init 0, depth 1: the raw predictions are -+2 learning_rate to the bit and equal scikit-learn's; train_score_ of the restatement
    and of scikit-learn lie inside the envelope at 1 ulp."""
    g = edges_golden()
    cuts = []
    for i, rate in enumerate(E.CUT_RATES):
        trees, score, raw, _ = E.fit_from(E.TWO_X, E.TWO_Y, 2, 1, E.EDGE_SEEDS, np.zeros(1), 1, rate)
        want = np.where(E.TWO_Y == 1, 2.0, -2.0) * rate
        assert np.array_equal(raw[:, 0], want) and np.array_equal(g["l%d_train_raw" % i][:, 0], want)
        cuts.append(float(want[-1]))
        for s in (score[0], g["l%d_train_score" % i][0]):
            fraction, inside, used = E.envelope_fraction(s, raw, E.TWO_Y, 2, E.E_HOST)
            assert inside, (rate, s, fraction)
    assert cuts == [2.0, 18.0, 33.3, 37.0, 40.0]
