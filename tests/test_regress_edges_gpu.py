"""Edges of the SVR bank kernel (kernels_svr.hpp) and of the forest-regressor kind (kernels_forest.hpp): seeded models against
the NumPy restatement (tests/svr_ref.py) over the smallest shapes at which the kernel takes another path -- around the
windows per workgroup, the models per workgroup and the support-vector tile (read from the library: paa_debug_svr_geometry).
Bound: |ours - restatement| <= 1e-9 max(1, scale(v)), scale(v) = sum_s |coef_s K_s(v)| + |intercept|."""
import numpy as np
import pytest

import svr_ref
from pyaudioanalysis_amd import _ffi, audioTrainTest

pytestmark = pytest.mark.gpu


def _geometry():
    geo = np.zeros(4, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_debug_svr_geometry(geo.ctypes.data_as(_ffi.c_i32p)))
    return int(geo[0]), int(geo[1]), int(geo[2])             # windows / workgroup, models / workgroup, tile


def _model(rng, n_sv, n_dims, kernel, gamma=None):
    sv = rng.standard_normal((n_sv, n_dims))
    coef = rng.standard_normal(n_sv)
    gamma = (1.0 / n_dims if gamma is None else gamma) if kernel == "rbf" else 0.0
    return (sv, coef, float(rng.standard_normal()), gamma, kernel)


def _arrays(m):
    return audioTrainTest.SvrArrays(m[0], m[1], [m[2]], m[3], m[4])


def _bank(models, means, stds):
    return audioTrainTest.SvrBank([_arrays(m) for m in models], means, stds)


def _check(models, feats, means, stds):
    got = _bank(models, means, stds).predict(feats)
    want, scale = svr_ref.bank_decision(models, feats, means, stds, with_scale=True)
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert np.all(err <= 1e-9 * np.maximum(1.0, scale)), (err.max(), scale.max())
    return got


def _stats(rng, n_models, n_dims):
    return rng.standard_normal((n_models, n_dims)) * 0.3, rng.uniform(0.5, 2.0, (n_models, n_dims))


def test_vector_counts_around_the_workgroup_and_a_padded_matrix(gpu_lib):
    W, _, tile = _geometry()
    rng = np.random.default_rng(1)
    models = [_model(rng, tile + 3, 9, "rbf"), _model(rng, 5, 9, "linear")]
    means, stds = _stats(rng, 2, 9)
    full = rng.standard_normal((9, 2 * W + 1))
    whole = _check(models, full, means, stds)
    for n in (1, 2, 3, W - 1, W, W + 1):
        part = _check(models, full[:, :n], means, stds)
        assert part.tobytes() == whole[:, :n].tobytes(), n                # a value does not depend on n_vec
    # ld > n_vec on the device path, and an output pitch of its own
    bank = _bank(models, means, stds)
    n, ld, ld_out = W + 1, 2 * W + 1, W + 7
    d_feats = _ffi.DeviceBuffer.from_host(full)
    d_out = _ffi.DeviceBuffer.from_host(np.full((2, ld_out), -7.0))
    try:
        bank.predict_device(d_feats, ld, n, d_out, ld_out)
        out = d_out.to_host(np.float64, 2 * ld_out).reshape(2, ld_out)
    finally:
        d_feats.free()
        d_out.free()
    assert out[:, :n].tobytes() == whole[:, :n].tobytes() and np.all(out[:, n:] == -7.0)
    assert bank.predict_device is not None and _ffi.lib().paa_svr_num_models(bank.handle) == 2


@pytest.mark.parametrize("n_dims", [1, 7, 8, 9, 136, 255, 256])
def test_dims(gpu_lib, n_dims):
    rng = np.random.default_rng(n_dims)
    models = [_model(rng, 19, n_dims, "rbf"), _model(rng, 19, n_dims, "linear")]
    means, stds = _stats(rng, 2, n_dims)
    _check(models, rng.standard_normal((n_dims, 5)), means, stds)


def test_support_vector_counts_around_the_tile(gpu_lib):
    _, _, tile = _geometry()
    rng = np.random.default_rng(2)
    feats = rng.standard_normal((11, 7))
    for kernel in ("rbf", "linear"):
        for n_sv in (0, 1, tile - 1, tile, tile + 1, 300):
            m = _model(rng, n_sv, 11, kernel)
            means, stds = _stats(rng, 1, 11)
            got = _check([m], feats, means, stds)
            if n_sv == 0:
                assert np.array_equal(got[0], np.full(7, m[2]))


def test_banks_around_the_model_chunk_are_the_single_models_bit_for_bit(gpu_lib):
    W, chunk, tile = _geometry()
    rng = np.random.default_rng(3)
    n_dims = 13
    feats = rng.standard_normal((n_dims, W + 3))
    # linear and RBF models with their own mean / std, a model without support vectors between two others, two
    # neighbours that share mean / std bit for bit (the kernel keeps their registers)
    kinds = ["rbf", "linear", "rbf", "rbf", "linear", "linear", "rbf"][:chunk + 3] + ["rbf"] * max(0, chunk - 4)
    sizes = [tile + 1, 3, 0, 2 * tile, 7, 0, 5] + [4] * max(0, chunk - 4)
    models = [_model(rng, s, n_dims, k) for k, s in zip(kinds, sizes)]
    means, stds = _stats(rng, len(models), n_dims)
    means[4], stds[4] = means[3], stds[3]
    assert len(models) >= chunk + 1
    singles = [_check([m], feats, means[i:i + 1], stds[i:i + 1])[0] for i, m in enumerate(models)]
    for n in (1, 2, 3, chunk + 1, len(models)):
        got = _check(models[:n], feats, means[:n], stds[:n])
        for i in range(n):
            assert got[i].tobytes() == singles[i].tobytes(), (n, i)
    again = _check(models, feats, means, stds)
    assert again.tobytes() == np.stack(singles).tobytes()                  # two runs are equal
    cols = [W + 2, 0, 5, W - 1]                                            # any sub-batch equals the same columns
    sub = _check(models, np.ascontiguousarray(feats[:, cols]), means, stds)
    assert sub.tobytes() == np.ascontiguousarray(again[:, cols]).tobytes()
    # zero-vector model between two others: exactly -rho
    assert np.array_equal(again[2], np.full(feats.shape[1], models[2][2]))


def test_extreme_gammas_and_a_query_on_a_support_vector(gpu_lib):
    rng = np.random.default_rng(4)
    n_dims = 10
    zeros, ones = np.zeros((1, n_dims)), np.ones((1, n_dims))
    feats = rng.standard_normal((n_dims, 6))
    tiny = _model(rng, 20, n_dims, "rbf", gamma=1e-300)                     # every K is exactly 1
    got = _check([tiny], feats, zeros, ones)
    huge = _model(rng, 20, n_dims, "rbf", gamma=1e300)                      # every K underflows to exactly 0
    got = _check([huge], feats, zeros, ones)
    assert np.array_equal(got[0], np.full(6, huge[2]))                      # ... and the prediction is exactly -rho
    feats[:, 2] = huge[0][7]                                                # a query equal to support vector 7: K = 1
    got = _check([huge], feats, zeros, ones)
    assert got[0, 2] == huge[1][7] + huge[2] and np.array_equal(np.delete(got[0], 2), np.full(5, huge[2]))


# ---- forest regressors ---------------------------------------------------------------------------------------------------
def _random_tree(rng, n_dims, depth):
    """A full binary tree of `depth` levels of splits in scikit-learn's arrays (depth 0: a single leaf)."""
    left, right, feat, thr, val, miss = [], [], [], [], [], []

    def grow(d):
        i = len(left)
        for a in (left, right, feat, thr, val, miss):
            a.append(0)
        val[i] = float(rng.standard_normal())
        if d == 0:
            left[i] = right[i] = -1
            feat[i], thr[i] = -2, -2.0
        else:
            feat[i], thr[i], miss[i] = int(rng.integers(0, n_dims)), float(rng.standard_normal() * 0.5), int(rng.integers(0, 2))
            left[i] = grow(d - 1)
            right[i] = grow(d - 1)
        return i
    grow(depth)
    return left, right, feat, thr, miss, val


def _forest(rng, n_trees, n_dims, depth):
    trees = [_random_tree(rng, n_dims, depth) for _ in range(n_trees)]
    cat = lambda k, dt: np.concatenate([np.asarray(t[k], dtype=dt) for t in trees])          # noqa: E731
    a = {"node_offsets": np.concatenate([[0], np.cumsum([len(t[0]) for t in trees])]).astype(np.int64),
         "children_left": cat(0, np.int64), "children_right": cat(1, np.int64), "feature": cat(2, np.int64),
         "threshold": cat(3, np.float64), "missing_go_to_left": cat(4, np.uint8), "value": cat(5, np.float64)}
    model = audioTrainTest.ForestArrays("regressor", a["node_offsets"], a["children_left"], a["children_right"], a["feature"],
                                        a["threshold"], a["missing_go_to_left"], a["value"], None, n_dims)
    return a, model


@pytest.mark.parametrize("n_trees,depth", [(1, 0), (1, 1), (4, 3), (5, 3), (100, 4)])
def test_forest_regressors_equal_the_restatement(gpu_lib, n_trees, depth):
    rng = np.random.default_rng(100 * n_trees + depth)
    n_dims = 6
    a, model = _forest(rng, n_trees, n_dims, depth)
    X = rng.standard_normal((70, n_dims))
    X[3, :] = np.nan                                                        # routed by missing_go_to_left at every split
    X[4, 2] = np.nan
    mean, std = rng.standard_normal(n_dims) * 0.1, rng.uniform(0.5, 2.0, n_dims)
    feats = (X * std + mean).T
    got = audioTrainTest.regress([model], "randomforest", feats, mean, std)[0]
    want = svr_ref.forest_regress(a, (feats.T - mean) / std)
    assert np.array_equal(got, want)
    idx, proba, raw = audioTrainTest.forest_model(model).predict(feats, mean, std, raw=True)
    assert proba.shape == (70, 1) and raw.shape == (70, 1) and np.all(idx == 0) and np.array_equal(raw[:, 0] / n_trees, got)
    bad = feats.copy()
    bad[1, 5] = 1e300
    with pytest.raises(ValueError, match=r"Input X contains infinity or a value too large for dtype\('float32'\)"):
        audioTrainTest.regress([model], "randomforest", bad, mean, std)
