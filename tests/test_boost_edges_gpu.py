"""GPU checks of the gradient-boosting fit at the edges its own suite (tests/test_boost_gpu.py) does not reach; the cases, the
references and their margins are in tests/boost_edge_cases.py and are established without a device by
tests/test_boost_edges_ref_cpu.py:
 (A) more than one row per thread in the sweep -- boost_gradient_kernel's chunks of ceil(n / 256) rows and the leaf step's over a
     leaf's rows: stage 0 of balanced jobs of 514, 1028 and 8192 rows and of 64 classes EQUAL to scikit-learn's, 255 / 256 / 257 rows
     against the restatement, a batch with one job above 256 rows among jobs below it (the whole fits above 256 rows run through
     the tests of test_boost_gpu.py, whose parametrisation they extend);
 (B) saturated and boundary raw predictions, through the `init` argument of paa_boost_fit_splits_f64: every range of log1pexp, both
     formulas of the binomial gradient, the 1e-150 guard of the leaf step and a softmax whose exponentials underflow, against true
     gradients and losses computed in mpmath; raw predictions that land exactly on the cuts;
 (C) learning rates and depths other than 0.1 and 3 in the sweep, and the builder's depth limit binding at kBoostMaxDepth = 20."""
import ctypes as C

import numpy as np
import pytest

import boost_edge_cases as E
import boost_ref as B
from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
from test_boost_cpu import FIELDS, GATE, rel, same_tree
from test_boost_edges_ref_cpu import edges_golden, near_fits, stage0_golden, table_jobs, whole_golden
from test_boost_gpu import model_trees, result_bytes, task_of, whole_job

pytestmark = pytest.mark.gpu

U = E.U


def fit_splits(X, labels, jobs, inits, stages, seeds, learning_rate, max_depth):
    """paa_boost_fit_splits_f64 itself (the Python wrapper fixes the learning rate, the depth and the init): jobs are lists of training
    rows (no test rows), inits [n_jobs][max_classes], stages and seeds (the rand_r seeds of a job's trees) per job; mean 0, scale 1.
    Returns per job a dict: score [stages], raw and resid [n][k_out], trees (dicts of arrays; stage-major, then class)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    inits = np.ascontiguousarray(inits, dtype=np.float64)
    n_jobs, d = len(jobs), X.shape[1]
    counts = [len(j) for j in jobs]
    k_out = [1 if len(np.unique(labels[j])) == 2 else len(np.unique(labels[j])) for j in jobs]
    n_trees = [int(stages[j]) * k_out[j] for j in range(n_jobs)]
    caps = [min(2 * counts[j] - 1, 2 ** (max_depth + 1) - 1) for j in range(n_jobs)]
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)          # noqa: E731
    train_off, train_idx = off(counts), np.concatenate(jobs).astype(np.int32)
    test_off, test_idx = np.zeros(n_jobs + 1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    mean, std = np.zeros((n_jobs, d)), np.ones((n_jobs, d))
    n_est = np.array(stages, dtype=np.int32)
    tree_seed = np.concatenate([np.asarray(seeds[j][:n_trees[j]], dtype=np.int64) for j in range(n_jobs)])
    assert tree_seed.shape[0] == sum(n_trees)
    score_off, raw_off = off(stages), off([counts[j] * k_out[j] for j in range(n_jobs)])
    node_off = off([n_trees[j] * caps[j] for j in range(n_jobs)])
    total = int(node_off[-1])
    score, raw, resid = np.zeros(int(score_off[-1])), np.zeros(int(raw_off[-1])), np.zeros(int(raw_off[-1]))
    i32, f64 = (lambda: np.zeros(total, dtype=np.int32)), (lambda: np.zeros(total))
    out = {"children_left": i32(), "children_right": i32(), "feature": i32(), "threshold": f64(), "impurity": f64(), "n_node_samples": i32(),
           "weighted_n_node_samples": f64(), "missing_go_to_left": np.zeros(total, dtype=np.uint8), "value": f64()}
    count = np.zeros(sum(n_trees), dtype=np.int32)
    label_out, flags, chunks = np.zeros(1, dtype=np.int32), np.zeros(n_jobs, dtype=np.int32), np.zeros(1, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_boost_fit_splits_f64(
        _ffi.as_f64p(X), X.shape[0], d, _ffi.as_i32p(labels), n_jobs, _ffi.as_i64p(train_off), _ffi.as_i32p(train_idx), _ffi.as_i64p(test_off),
        _ffi.as_i32p(test_idx), _ffi.as_f64p(mean), _ffi.as_f64p(std), _ffi.as_i32p(n_est), _ffi.as_i64p(tree_seed), _ffi.as_f64p(inits),
        inits.shape[1], float(learning_rate), int(max_depth), 0, _ffi.as_i32p(label_out), None, _ffi.as_f64p(score), _ffi.as_f64p(raw),
        _ffi.as_f64p(resid), total, _ffi.as_i32p(count), _ffi.as_i32p(out["children_left"]), _ffi.as_i32p(out["children_right"]),
        _ffi.as_i32p(out["feature"]), _ffi.as_f64p(out["threshold"]), _ffi.as_f64p(out["impurity"]), _ffi.as_i32p(out["n_node_samples"]),
        _ffi.as_f64p(out["weighted_n_node_samples"]), out["missing_go_to_left"].ctypes.data_as(C.POINTER(C.c_uint8)), _ffi.as_f64p(out["value"]),
        _ffi.as_i32p(flags), _ffi.as_i32p(chunks)))
    assert not flags.any()
    res, t0 = [], 0
    for j in range(n_jobs):
        trees = []
        for t in range(n_trees[j]):
            lo = int(node_off[j]) + t * caps[j]
            tree = {f: out[f][lo:lo + int(count[t0 + t])] for f in FIELDS}
            tree["value"] = tree["value"].reshape(-1, 1)
            trees.append(tree)
        t0 += n_trees[j]
        shape = (counts[j], k_out[j])
        res.append(dict(score=score[int(score_off[j]):int(score_off[j + 1])], raw=raw[int(raw_off[j]):int(raw_off[j + 1])].reshape(shape),
                        resid=resid[int(raw_off[j]):int(raw_off[j + 1])].reshape(shape), trees=trees))
    return res


# ---- (A) more than one row per thread ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.STAGE0))
def test_stage_0_above_256_rows_equals_scikit_learn(gpu_lib, name):
    """The acceptance of test_stage_0_of_balanced_jobs_equals_scikit_learn at 514, 1028 and 8192 rows (chunks of 3, 5 and 32 rows per
    thread in the gradient kernel, leaves above 256 rows in the leaf step) and at 64 classes: tree arrays, Newton leaf values, init and
    the raw predictions bit for bit, train_score_ to the gate."""
    g, p, X, y, K, rs = stage0_golden(name)
    res = aT.boosting_split_fit_predict(X, y, [whole_job(X, np.arange(len(y)), np.zeros(0, dtype=int), 1, rs)], train_score=True, trees=True)
    m = res.models[0]
    assert np.array_equal(m.init, g[p + "init"]) and np.array_equal(res.train_raw[0], g[p + "train_raw"])
    print("%s: train_score_ within %.3g (relative)" % (name, rel(res.train_score[0], g[p + "train_score"])))
    assert rel(res.train_score[0], g[p + "train_score"]) <= GATE
    trees = model_trees(m)
    assert len(trees) == (1 if K == 2 else K)
    for t, tree in enumerate(trees):
        lo, hi = int(g[p + "node_offsets"][t]), int(g[p + "node_offsets"][t + 1])
        for f in FIELDS:
            want = g[p + f][lo:hi]
            assert np.asarray(tree[f]).reshape(-1).astype(want.dtype).tobytes() == want.tobytes(), (name, t, f)


@pytest.mark.parametrize("name", list(E.NEAR_256))
def test_either_side_of_one_row_per_thread(gpu_lib, name):
    """255, 256 and 257 rows (the last unbalanced), one call with a 1-stage and a 2-stage job, against the restatement: the same tree
    structures, train_score_ and raw predictions to the gate, the gradients of both stages within 4 x 2^-52 of the host's; with 256
    balanced rows the init is 0 and stage 0 is exact: leaf values and raw predictions bit for bit."""
    X, y, K, rs, seeds, want, _ = near_fits(name)
    none = np.zeros(0, dtype=np.int64)
    res = aT.boosting_split_fit_predict(X, y, [whole_job(X, np.arange(len(y)), none, s, rs) for s in (1, 2)], train_score=True, trees=True)
    trees = model_trees(res.models[1])
    assert len(trees) == 2
    for got, ref in zip(trees, want[0]):
        for f in ("children_left", "children_right", "feature", "threshold", "n_node_samples"):
            assert np.array_equal(np.asarray(got[f]).reshape(-1), np.asarray(ref[f]).reshape(-1)), (name, f)
        assert rel(got["value"], ref["value"]) <= GATE
    assert np.array_equal(res.models[1].init, want[3])
    assert rel(res.train_score[1], want[1]) <= GATE and rel(res.train_raw[1], want[2]) <= GATE
    assert res.train_score[0][0] == res.train_score[1][0]
    raw0 = np.tile(want[3], (len(y), 1))
    worst = max(float(np.max(np.abs(res.train_resid[0] - B.gradient_and_loss(raw0, y, K)[0]))),
                float(np.max(np.abs(res.train_resid[1] - B.gradient_and_loss(res.train_raw[0], y, K)[0]))))
    print("%s: the device's gradients within %.2f ulp of 1 of the host's" % (name, worst * 2.0 ** 52))
    assert worst <= 4 * U
    if name == "rows_256":
        one = B.fit(X, y, K, 1, seeds)
        assert np.array_equal(res.train_raw[0], one[2]) and np.array_equal(model_trees(res.models[0])[0]["value"], one[0][0]["value"])


def batch_jobs():
    """boost_edge_cases.batch_specs() over one matrix of 12 dims: 150, 777 and 240 training rows with 2, 3 and 1 stages and 2, 3 and 8
    classes."""
    parts, jobs, ys, at = [], [], [], 0
    for name, stages in E.batch_specs():
        X, y, tr, te, K, _, rs = (E if name in E.WHOLE else B).whole_case(name)
        Xp = np.zeros((X.shape[0], 12))
        Xp[:, :X.shape[1]] = X
        Xp[:, X.shape[1]:] = np.random.RandomState(K).randn(X.shape[0], 12 - X.shape[1]).astype(np.float32)
        parts.append(Xp)
        ys.append(y + 10 * len(jobs))
        jobs.append((tr + at, te + at, Xp[tr].mean(0), Xp[tr].std(0), (stages, rs)))
        at += X.shape[0]
    return np.concatenate(parts), np.concatenate(ys), jobs


def test_same_bits_with_a_job_above_256_rows_among_smaller_ones(gpu_lib):
    """test_same_bits_alone_in_a_batch_and_across_chunks with n_max = 777 above the other jobs' 150 and 240 rows and stage counts
    2, 3, 1: the jobs of stages 1 and 2 are strict prefixes of the chunk's order (777, 150, 240 rows)."""
    X, y, jobs = batch_jobs()
    assert [len(j[0]) for j in jobs] == [150, 777, 240] and [j[4][0] for j in jobs] == [2, 3, 1]
    both = aT.boosting_split_fit_predict(X, y, jobs, proba=True, train_score=True, trees=True)
    assert both.n_chunks == 1 and [len(c) for c in both.classes] == [2, 3, 8]
    for j in range(3):
        alone = aT.boosting_split_fit_predict(X, y, [jobs[j]], proba=True, train_score=True, trees=True)
        assert result_bytes(alone, 0) == result_bytes(both, j), j
        assert both.models[j].node_offsets.shape[0] - 1 == jobs[j][4][0] * (1 if len(both.classes[j]) == 2 else len(both.classes[j]))
    chunked = aT.boosting_split_fit_predict(X, y, jobs, proba=True, train_score=True, trees=True, chunk_bytes=128 * 1024)
    assert chunked.n_chunks >= 2
    for j in range(3):
        assert result_bytes(chunked, j) == result_bytes(both, j), j


# ---- (B) saturated and boundary raw predictions ------------------------------------------------------------------------------------------

_TABLES = {}


def table(K):
    """ONE call per class count: every init of the table with 1 stage, then with 2.  [(init row, stages, the job's result)]"""
    if K not in _TABLES:
        X, y = E.edge_inputs(K)
        jobs = table_jobs(K)
        res = fit_splits(X, y, [np.arange(len(y))] * len(jobs), np.array([init for init, _ in jobs]), [s for _, s in jobs],
                         [E.EDGE_SEEDS] * len(jobs), E.EDGE_RATE, E.EDGE_DEPTH)
        _TABLES[K] = [(init, s, r) for (init, s), r in zip(jobs, res)]
    return _TABLES[K]


def raw_before_last_stage(K, init, stages):
    """What the gradients of a job's last stage were formed from: its init, or the raw predictions the 1-stage job of the same init
    returned (the first stage of a job is the same model: the batch test)."""
    X, y = E.edge_inputs(K)
    k_out = 1 if K == 2 else K
    if stages == 1:
        return np.tile(init[:k_out], (len(y), 1))
    return next(r["raw"] for i, s, r in table(K) if s == 1 and np.array_equal(i, init))


@pytest.mark.parametrize("K", (2, 3))
def test_gradients_at_saturated_and_boundary_raw_predictions(gpu_lib, K):
    """Every element of train_resid against the true y - sigmoid(raw) / (y == k) - softmax(raw)[k] in mpmath: within 4 x 2^-52 of the
    true value's own magnitude (boost_edge_cases.gradient_ratio: equality where the truth is exactly 0 or +-1; for the softmax
    gradient of a row's own class, which the formula forms as 1 - p_y, of the larger of the truth and p_y), for the 1-stage jobs from
    the init and for the 2-stage jobs from the raw predictions stage 0 returned; everything returned is finite."""
    X, y = E.edge_inputs(K)
    worst = 0.0
    for init, stages, r in table(K):
        assert np.all(np.isfinite(r["resid"])) and np.all(np.isfinite(r["raw"])) and np.all(np.isfinite(r["score"])), (init, stages)
        assert all(np.all(np.isfinite(t["value"])) for t in r["trees"]), (init, stages)
        ratio = E.worst_gradient_ratio(r["resid"], raw_before_last_stage(K, init, stages), y, K)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (init, stages, ratio * E.GRAD_ULPS)
    print("K = %d: the device's gradients within %.3f of the bound (%.2f x 2^-52 relative to the true value)" % (K, worst, worst * E.GRAD_ULPS))


@pytest.mark.parametrize("K", (2, 3))
def test_leaf_steps_at_saturated_and_boundary_raw_predictions(gpu_lib, K):
    """The leaf step replayed from the device's OWN gradients, which needs no exp: every leaf value of a job's last stage is
    boost_ref.leaf_value of train_resid over the leaf's rows -- bit for bit where the leaf's residuals are all equal or the leaf is the
    root (the order of the sum is then immaterial or the row order), else within the bound of the traced replay -- and the raw
    predictions are those before the stage plus learning_rate x value, to the bit.  Outside the cliff bands near +-37 the 1-stage
    trees equal the restatement's: two pure leaves, 0.0 where den is exactly 0 or below 1e-150, -1 / 0 at -40, -+2 at 0."""
    X, y = E.edge_inputs(K)
    x32 = X.astype(np.float32)
    k_out = 1 if K == 2 else K
    factor = 1.0 if K == 2 else (K - 1) / K
    for init, stages, r in table(K):
        before = raw_before_last_stage(K, init, stages)
        want_raw = before.copy()
        for k in range(k_out):
            tree = r["trees"][(stages - 1) * k_out + k]
            yk = (y == (1 if K == 2 else k)).astype(np.float64)
            for node, rows in E.leaf_rows(tree, x32).items():
                assert tree["children_left"][node] < 0 and int(tree["n_node_samples"][node]) == len(rows)
                res = r["resid"][rows, k]
                v, got = float(B.leaf_value(res, yk[rows], K)), float(tree["value"][node, 0])
                if node == 0 or np.all(res == res[0]):
                    assert got == v, (init, stages, k, node, got, v)
                else:
                    pr = yk[rows] - res
                    nn, num, den = len(rows), float(np.sum(res)), float(np.sum(pr * (1.0 - pr)))
                    e_num, e_den = nn * U * np.abs(res).sum(), nn * U * np.abs(pr * (1.0 - pr)).sum()
                    assert abs(den) / nn >= 1e-140 and abs(got - v) <= (factor * e_num + abs(v) * e_den) / (abs(den) - e_den) + 8 * U * abs(v), (init, stages, k, node)
                want_raw[rows, k] = before[rows, k] + E.EDGE_RATE * got
        assert np.array_equal(r["raw"], want_raw), (init, stages)
        if stages == 1 and not E.job_in_cliff(before, y):
            ref = E.edge_fit(K, init, 1)[0]
            for k in range(k_out):
                for f in ("children_left", "children_right", "feature", "threshold", "n_node_samples"):
                    assert np.array_equal(r["trees"][k][f], ref[k][f]), (init, k, f)
    if K == 2:
        leaves = {float(init[0]): (float(r["trees"][0]["value"][1, 0]), float(r["trees"][0]["value"][2, 0]), r) for init, s, r in table(2) if s == 1}
        for init, want in ((0.0, (-2.0, 2.0)), (40.0, (0.0, 0.0)), (700.0, (0.0, 0.0)), (-40.0, (-1.0, 0.0)), (-700.0, (0.0, 0.0)), (-720.0, (0.0, 0.0))):
            ref = E.edge_fit(2, np.array([init, 0.0]), 1)[0][0]["value"]
            assert leaves[init][:2] == want == (float(ref[1, 0]), float(ref[2, 0])), (init, leaves[init][:2])
        for init in (40.0, 700.0, -700.0, -720.0):                     # den exactly 0 or below 1e-150: the raw predictions stay
            assert np.all(leaves[init][2]["raw"] == init)
        assert leaves[40.0][2]["score"][0] == 50.0                     # 2 (5 x 40 + 3 x 0) / 8
    else:
        for i in E.THREE_SATURATED:
            init, loss = E.THREE_INITS[i]
            for stages in (1, 2):
                r = next(r for j, s, r in table(3) if s == stages and tuple(j) == init)
                assert all(np.all(t["value"][t["children_left"] < 0] == 0.0) for t in r["trees"]), init
                assert np.array_equal(r["raw"], np.tile(init, (9, 1))) and np.all(r["score"] == loss), (init, r["score"])


@pytest.mark.parametrize("K", (2, 3))
def test_losses_at_saturated_and_boundary_raw_predictions(gpu_lib, K):
    """train_score_ of the last stage against the returned raw predictions: inside the envelope of scikit-learn's formula
    (boost_edge_cases.loss_envelope) at E_DEVICE ulp per exp / log / log1p; train_score_[0] of a 2-stage job is the 1-stage job's, to
    the bit.  The jobs in the cliff bands are left to the gradient test."""
    X, y = E.edge_inputs(K)
    k_out = 1 if K == 2 else K
    worst, most = 0.0, 0.0
    for init, stages, r in table(K):
        if E.job_in_cliff(np.tile(init[:k_out], (len(y), 1)), y):
            continue
        fraction, inside, used = E.envelope_fraction(r["score"][-1], r["raw"], y, K, E.E_DEVICE)
        worst, most = max(worst, fraction), max(most, used)
        assert inside, (init, stages, float(r["score"][-1]), fraction)
        if stages == 2:
            one = next(q for i, s, q in table(K) if s == 1 and np.array_equal(i, init))
            assert r["score"][0] == one["score"][0], (init, r["score"], one["score"])
    print("K = %d: train_score_ within %.3f of the envelope's reach from the true mean loss and %.3f of its half width from its middle, at %d ulp"
          % (K, worst, most, E.E_DEVICE))


def test_raw_predictions_that_land_on_the_cuts(gpu_lib):
    """init 0, depth 1, learning rates 1, 9, 16.65, 18.5 and 20: the leaves are -+2, the raw predictions -+2, -+18, -+33.3, -+37 and
    -+40 to the bit (scikit-learn's with init="zero"); train_score_ inside the envelope."""
    g = edges_golden()
    worst = 0.0
    for i, rate in enumerate(E.CUT_RATES):
        r = fit_splits(E.TWO_X, E.TWO_Y, [np.arange(8)], np.zeros((1, 2)), [1], [E.EDGE_SEEDS], rate, 1)[0]
        assert [float(v) for v in r["trees"][0]["value"][1:, 0]] == [-2.0, 2.0]
        assert r["raw"].tobytes() == g["l%d_train_raw" % i].tobytes() and np.array_equal(r["raw"][:, 0], np.where(E.TWO_Y == 1, 2.0, -2.0) * rate)
        fraction, inside, used = E.envelope_fraction(r["score"][0], r["raw"], E.TWO_Y, 2, E.E_DEVICE)
        worst = max(worst, fraction)
        print("rate %g: train_score_ %.17g (scikit-learn %.17g), %.3f of the envelope's reach, %.3f of its half width"
              % (rate, r["score"][0], g["l%d_train_score" % i][0], fraction, used))
        assert inside, (rate, float(r["score"][0]), fraction)


# ---- (C) other learning rates and depths ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.PARAMS))
def test_whole_fits_under_other_learning_rates_and_depths(gpu_lib, name):
    """(learning_rate, max_depth) = (1, 1), (0.5, 2) and (0.1, 20) on the 300-row job, 3 stages: train_score_ and the raw predictions
    within 1e-9 of scikit-learn's, every tree's node count equal to scikit-learn's (depth 20: grown until the leaves are pure)."""
    g, p, X, y, tr, te, K, stages, rs = whole_golden(name)
    rate, depth = E.PARAMS[name]
    r = fit_splits(X, y, [tr], np.array([[float(g[p + "init"][0]), 0.0]]), [stages], [g[p + "seeds"].tolist()], rate, depth)[0]
    score, raw = rel(r["score"], g[p + "train_score"]), rel(r["raw"], g[p + "train_raw"])
    print("%s: train_score_ within %.3g, training raw predictions within %.3g (relative)" % (name, score, raw))
    assert score <= GATE and raw <= GATE
    assert [t["feature"].shape[0] for t in r["trees"]] == g[p + "node_count"].tolist()
    # the stage-0 tree is what CART demands in exact arithmetic under THIS depth limit, for the host's gradients at the init (the
    # device's are within 4 x 2^-52 of them).  The later trees are not compared with the restatement's node by node: its libm is not
    # the device's, and where two splits tie in exact arithmetic (depth 20 meets such nodes) an ulp decides which comes first
    resid = B.gradient_and_loss(np.tile(g[p + "init"], (len(tr), 1)), y[tr], K)[0]
    B.check_boost_stage(r["trees"][0], X[tr].astype(np.float32), resid[:, 0], np.ones(len(tr), dtype=np.int64), depth, y_err=4 * U)


def test_builder_at_the_depth_limit_of_20(gpu_lib):
    """The chain of 22 one-hot rows: under max_depth = 20 the tree equals scikit-learn's -- 41 nodes, the leaf at depth 20 holds 2 rows
    and is impure --, under 21 it is the pure chain of 43 nodes."""
    g = edges_golden()
    for depth, nodes in ((20, 41), (21, 43)):
        c = E.chain_case(depth)
        tree = aT.tree_fit_boosting(c["X"], [task_of(c)], max_depth=depth).trees[0]
        same_tree(tree, g, "chain%d_" % depth, "chain %d" % depth)
        assert tree["feature"].shape[0] == nodes
    assert g["chain20_impurity"][20] > 0.05 and g["chain20_n_node_samples"][20] == 2 and np.all(g["chain21_impurity"][g["chain21_children_left"] < 0] == 0.0)
