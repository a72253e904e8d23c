"""NumPy restatement of what the regression kernels compute (kernels_svr.hpp, the regressor kind of kernels_forest.hpp) and
of the reference's evaluate_regression (audioTrainTest.py:774-855) over a `predict` callable.  Test infrastructure only."""
import io
import contextlib

import numpy as np


def svr_arrays(model):
    """(support vectors, coefficients, intercept, gamma, kernel) of a fitted sklearn.svm.SVR or SvrArrays-like object."""
    return (np.asarray(model.support_vectors_, dtype=np.float64), np.asarray(model._dual_coef_, dtype=np.float64).reshape(-1),
            float(np.asarray(model._intercept_).reshape(-1)[0]), float(model._gamma), str(model.kernel))


def kernel_values(sv, gamma, kernel, X):
    """K[s][v] of standardised rows X [n_vec][n_dims]: libsvm's dense k_function (RBF in the difference form)."""
    if sv.shape[0] == 0:
        return np.zeros((0, X.shape[0]))
    if kernel == "rbf":
        d = sv[:, None, :] - X[None, :, :]
        return np.exp(-gamma * np.einsum("svd,svd->sv", d, d))
    return sv @ X.T


def svr_decision(sv, coef, intercept, gamma, kernel, X, with_scale=False):
    """libsvm's svm_predict_values for an epsilon-SVR: sum_s coef[s] K_s in the model's order, minus rho (= plus the
    intercept); with_scale: also scale(v) = sum_s |coef_s K_s(v)| + |intercept|, the size of the terms that are added."""
    K = kernel_values(sv, gamma, kernel, X)
    acc = np.zeros(X.shape[0])
    scale = np.zeros(X.shape[0])
    for s in range(sv.shape[0]):
        acc = acc + coef[s] * K[s]
        scale = scale + np.abs(coef[s] * K[s])
    out = acc - (-intercept)
    return (out, scale + abs(intercept)) if with_scale else out


def standardise(feats, mean, std):
    """feats [n_dims][n_vec] -> rows [n_vec][n_dims] of (x - mean) / std."""
    return (np.asarray(feats, dtype=np.float64).T - mean) / std


def bank_decision(models, feats, means, stds, with_scale=False):
    """[n_models][n_vec] for models given as svr_arrays tuples, feats [n_dims][n_vec], one mean / std row per model."""
    rows = [svr_decision(*m, standardise(feats, means[i], stds[i]), with_scale=with_scale) for i, m in enumerate(models)]
    if with_scale:
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    return np.stack(rows)


def forest_regress(a, X):
    """RandomForestRegressor.predict (n_jobs=None) from concatenated tree arrays `a` (node_offsets, children_left,
    children_right, feature, threshold, missing_go_to_left, value [nodes]) on standardised rows X: the float32 cast of the
    input, 0.0 + v_0 + v_1 + ... in tree order, divided by the number of trees."""
    X32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    n_trees = len(a["node_offsets"]) - 1
    out = np.zeros(X32.shape[0])
    for v in range(X32.shape[0]):
        acc = 0.0
        for t in range(n_trees):
            base = int(a["node_offsets"][t])
            n = 0
            while a["children_left"][base + n] != -1:
                x = X32[v, a["feature"][base + n]]
                left = bool(a["missing_go_to_left"][base + n]) if np.isnan(x) else np.float64(x) <= a["threshold"][base + n]
                n = int(a["children_left"][base + n] if left else a["children_right"][base + n])
            acc = acc + float(a["value"][base + n])
        out[v] = acc / n_trees
    return out


def evaluate_regression(features, labels, n_exp, method_name, params, fit, predict):
    """The reference's evaluate_regression with fit(train rows, train labels, method, param) -> model and
    predict(model, rows) -> values in place of scikit-learn's calls: np.random.permutation consumed per experiment, a
    90 / 10 split, squared test error, absolute training error, the mean-label baseline.  Returns ((best param, its error,
    its baseline error), printed table)."""
    from sklearn.preprocessing import StandardScaler
    X = StandardScaler().fit_transform(features)
    labels = np.asarray(labels)
    n = labels.shape[0]
    n_train = int(round(0.9 * n))
    e_all, t_all, b_all = [], [], []
    for param in params:
        errs, terrs, berrs = [], [], []
        for _ in range(n_exp):
            perm = np.random.permutation(range(n))
            tr, te = perm[:n_train], perm[n_train:]
            l_train = [labels[i] for i in tr]
            model = fit(X[tr], l_train, method_name, param)
            terrs.append(np.mean(np.abs(predict(model, X[tr]) - l_train)))
            R = predict(model, X[te])
            base = np.mean(l_train)
            errs.append(np.array([(R[k] - labels[i]) * (R[k] - labels[i]) for k, i in enumerate(te)]).mean())
            berrs.append(np.array([(base - labels[i]) * (base - labels[i]) for i in te]).mean())
        e_all.append(np.array(errs).mean())
        t_all.append(np.array(terrs).mean())
        b_all.append(np.array(berrs).mean())
    best = int(np.argmin(e_all))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        print("{0:s}\t\t{1:s}\t\t{2:s}\t\t{3:s}".format("Param", "MSE", "T-MSE", "R-MSE"))
        for i in range(len(e_all)):
            print("{0:.4f}\t\t{1:.2f}\t\t{2:.2f}\t\t{3:.2f}".format(params[i], e_all[i], t_all[i], b_all[i]), end="")
            print("\t\t best" if i == best else "")
    return (params[best], e_all[best], b_all[best]), out.getvalue()


def sklearn_fit(rows, labels, method_name, param):
    """The reference's trainers (audioTrainTest.py:222-233) without their training-error pass."""
    import sklearn.ensemble
    import sklearn.svm
    if method_name == "randomforest":
        return sklearn.ensemble.RandomForestRegressor(n_estimators=param).fit(rows, labels)
    return sklearn.svm.SVR(C=param, kernel="rbf" if method_name == "svm_rbf" else "linear").fit(rows, labels)


def tree_arrays(model):
    """Concatenated tree_ arrays of a fitted RandomForestRegressor, as forest_regress reads them."""
    parts = [t.tree_ for t in model.estimators_]
    cat = lambda get: np.concatenate([np.asarray(get(p)) for p in parts])          # noqa: E731
    return {"node_offsets": np.concatenate([[0], np.cumsum([p.node_count for p in parts])]).astype(np.int64),
            "children_left": cat(lambda p: p.children_left), "children_right": cat(lambda p: p.children_right),
            "feature": cat(lambda p: p.feature), "threshold": cat(lambda p: p.threshold),
            "missing_go_to_left": cat(lambda p: getattr(p, "missing_go_to_left", np.zeros(p.node_count, dtype=np.uint8))),
            "value": cat(lambda p: np.asarray(p.value, dtype=np.float64).reshape(p.node_count, -1)[:, 0])}
