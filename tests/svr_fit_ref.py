"""NumPy FP64 restatement of the batched epsilon-SVR solver and of the SVR split sweep (pyaudioanalysis_amd/csrc/kernels_svrfit.hpp;
audioTrainTest.svr_solve / svr_split_fit_predict / evaluate_regression(svm_fit="device")) -- the CPU second opinion of the GPU
kernel.  Test helper, not part of the package.

solve() is libsvm's solve_epsilon_svr over its Solver without shrinking (sklearn/svm/src/libsvm/svm.cpp: Solver::Solve,
select_working_set, calculate_rho) on a precomputed n x n Gram matrix, in float64 throughout (libsvm keeps its kernel cache in
float32).  The dual has 2 n variables: variable v stands for row v mod n, its sign is +1 for v < n and -1 for v >= n, its linear
term epsilon - y for v < n and epsilon + y for v >= n, and Q_uv = sign_u sign_v K[u mod n, v mod n]."""
import numpy as np

from smo_ref import STATUS_CONVERGED, STATUS_NOT_CONVERGED, TAU, gap_and_sets, gram, rho_of

SVR_EPSILON = 0.1           # scikit-learn's default, which train_svm_regression leaves in place


def dual_signs(n):
    return np.concatenate([np.ones(n), -np.ones(n)])


def solve(K, targets, C, epsilon=SVR_EPSILON, eps=1e-3, max_iter=10**7):
    """(alpha [2 n], G [2 n], rho, iterations, gap, status) of min 1/2 a^T Q a + p^T a, 0 <= a <= C, s^T a = 0."""
    t = np.asarray(targets, dtype=np.float64)
    n = t.shape[0]
    s = dual_signs(n)
    alpha, G = np.zeros(2 * n), np.concatenate([epsilon - t, epsilon + t])
    QD = np.concatenate([np.diagonal(K), np.diagonal(K)])
    it, idx = 0, np.arange(2 * n)
    while True:
        gmax, gmax2, up, low, v = gap_and_sets(alpha, G, s, C)
        if not up.any() or gmax + gmax2 < eps:
            status = STATUS_CONVERGED
            break
        if it >= max_iter:
            status = STATUS_NOT_CONVERGED
            break
        cand_i = idx[up]
        vi = v[up]
        i = int(cand_i[vi.shape[0] - 1 - int(np.argmax(vi[::-1]))])       # the greatest index attaining the maximum
        Ki = np.concatenate([K[i % n], K[i % n]])
        b = gmax - v
        cand = low & (b > 0)
        if not cand.any():
            status = STATUS_CONVERGED
            break
        eta = QD[i] + QD - 2.0 * Ki
        eta = np.where(eta > 0, eta, TAU)
        obj = np.where(cand, -(b * b) / eta, np.inf)
        j = 2 * n - 1 - int(np.argmin(obj[::-1]))
        ai, aj = alpha[i], alpha[j]
        if s[i] != s[j]:
            delta = (-G[i] - G[j]) / eta[j]
            d = ai - aj
            ni, nj = ai + delta, aj + delta
            if d > 0 and nj < 0:
                nj, ni = 0.0, d
            elif d <= 0 and ni < 0:
                ni, nj = 0.0, -d
            if d > 0 and ni > C:
                ni, nj = C, C - d
            elif d <= 0 and nj > C:
                nj, ni = C, C + d
        else:
            delta = (G[i] - G[j]) / eta[j]
            sm = ai + aj
            ni, nj = ai - delta, aj + delta
            if sm > C and ni > C:
                ni, nj = C, sm - C
            elif sm <= C and nj < 0:
                nj, ni = 0.0, sm
            if sm > C and nj > C:
                nj, ni = C, sm - C
            elif sm <= C and ni < 0:
                ni, nj = 0.0, sm
        Kj = np.concatenate([K[j % n], K[j % n]])
        G += s * (Ki * (s[i] * (ni - ai)) + Kj * (s[j] * (nj - aj)))
        alpha[i], alpha[j] = ni, nj
        it += 1
    gap = gmax + gmax2 if np.isfinite(gmax) and np.isfinite(gmax2) else 0.0
    return alpha, G, rho_of(alpha, G, s, C), it, float(gap), status


def gradient(K, targets, alpha, epsilon=SVR_EPSILON):
    """G = Q alpha + p recomputed from alpha alone."""
    t = np.asarray(targets, dtype=np.float64)
    n = t.shape[0]
    kb = K @ (alpha[:n] - alpha[n:])
    return np.concatenate([kb + epsilon - t, -kb + epsilon + t])


def scale_gamma(Z):
    """scikit-learn's gamma='scale' for the standardised training rows Z."""
    var = Z.var()
    return 1.0 / (Z.shape[1] * var) if var != 0 else 1.0


def fit_job(X, y, job, kernel="linear", gamma=None, epsilon=SVR_EPSILON, eps=1e-3, max_iter=10**7):
    """One job (train_idx, test_idx, mean, scale, C): (test predictions, training predictions from the final gradient, beta, rho,
    iterations, status, n_sv, gamma)."""
    train_idx, test_idx, mean, scale, C = job
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    tr = np.asarray(train_idx, dtype=np.int64)
    Z = (X[tr] - mean) / scale
    Zq = (X[np.asarray(test_idx, dtype=np.int64)] - mean) / scale
    if gamma is None:
        gamma = scale_gamma(Z) if kernel == "rbf" else 1.0
    n = tr.shape[0]
    alpha, G, rho, it, _, status = solve(gram(Z, kernel, gamma), y[tr], float(C), epsilon, eps, max_iter)
    beta = alpha[:n] - alpha[n:]
    sv = beta != 0
    pred = gram(Zq, kernel, gamma, Z[sv]) @ beta[sv] - rho
    return pred, G[:n] - epsilon + y[tr] - rho, beta, rho, it, status, int(np.count_nonzero(sv)), gamma


def evaluate_regression_ref(features, labels, n_exp, method_name, params, fit=None):
    """What evaluate_regression computes, on the CPU: per parameter value n_exp permutations from NumPy's global state, 90 / 10
    splits of the standardised samples, the errors of audioTrainTest.py:774-855.  fit(Z, y, train, test, param) returns (test
    predictions, training predictions); None: the restatement, i.e. what svm_fit="device" computes (an SVR fit draws nothing from
    the global state, so drawing every permutation up front gives the same splits).  Returns (best parameter, its error, its
    baseline error, errors per parameter, training errors per parameter)."""
    X = np.asarray(features, dtype=np.float64)
    labels = np.asarray(labels)
    Z = (X - X.mean(axis=0)) / X.std(axis=0)            # StandardScaler
    n = labels.shape[0]
    n_train = int(round(0.9 * n))
    kernel = "rbf" if method_name == "svm_rbf" else "linear"
    zeros, ones = np.zeros(X.shape[1]), np.ones(X.shape[1])
    if fit is None:
        def fit(Zs, ys, train, test, param):
            return fit_job(Zs, ys, (train, test, zeros, ones, param), kernel)[:2]
    errors_all, train_all, base_all = [], [], []
    for param in params:
        errors, errors_train, errors_base = [], [], []
        for _ in range(n_exp):
            perm = np.random.permutation(range(n))
            train, test = perm[:n_train], perm[n_train:]
            pred_test, pred_train = fit(Z, labels, train, test, param)
            baseline = np.mean(labels[train])
            errors.append(np.mean((pred_test - labels[test]) ** 2))
            errors_base.append(np.mean((baseline - labels[test]) ** 2))
            errors_train.append(np.mean(np.abs(pred_train - labels[train])))
        errors_all.append(np.mean(errors))
        train_all.append(np.mean(errors_train))
        base_all.append(np.mean(errors_base))
    best = int(np.argmin(errors_all))
    return params[best], errors_all[best], base_all[best], np.array(errors_all), np.array(train_all)
