"""NumPy restatement of libsvm's svm_predict_values / svm_predict / svm_predict_probability as scikit-learn runs them
(sklearn/svm/src/libsvm/svm.cpp, dense representation) -- the CPU second opinion for the GPU SVC kernel
(pyaudioanalysis_amd/csrc/kernels_svc.hpp).  Test helper, not part of the package.

The model is given as the arrays scikit-learn keeps (see model_arrays): libsvm's sv_coef is SVC._dual_coef_ and its rho is
-SVC._intercept_; the public dual_coef_ / intercept_ have the opposite sign for two classes."""
import numpy as np


def model_arrays(clf):
    """The arrays of a fitted sklearn SVC in libsvm's layout."""
    kernel = clf.kernel
    if kernel not in ("rbf", "linear"):
        raise NotImplementedError(kernel)
    return {
        "support_vectors": np.ascontiguousarray(clf.support_vectors_, dtype=np.float64),
        "n_support": np.asarray(clf.n_support_, dtype=np.int32),
        "dual_coef": np.ascontiguousarray(clf._dual_coef_, dtype=np.float64),
        "rho": -np.asarray(clf._intercept_, dtype=np.float64),
        "prob_a": np.asarray(clf.probA_, dtype=np.float64),
        "prob_b": np.asarray(clf.probB_, dtype=np.float64),
        "gamma": float(clf._gamma) if kernel == "rbf" else 0.0,
        "kernel": kernel,
    }


def kernel_values(m, X):
    """K[v, s] for vectors X [n_vec][n_dims] (already standardised)."""
    sv = m["support_vectors"]
    if m["kernel"] == "rbf":
        d2 = np.empty((X.shape[0], sv.shape[0]))
        for v in range(X.shape[0]):                       # difference form, as libsvm's dense k_function
            diff = sv - X[v]
            d2[v] = np.einsum("sd,sd->s", diff, diff)
        return np.exp(-m["gamma"] * d2)
    return X @ sv.T


def decision_values(m, X):
    """libsvm's dec_values [n_vec][k (k - 1) / 2], pairs (i, j), i < j, in row-major order."""
    K = kernel_values(m, X)
    ns = np.asarray(m["n_support"], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(ns)])
    k = len(ns)
    coef = m["dual_coef"]
    out = np.empty((X.shape[0], k * (k - 1) // 2))
    p = 0
    for i in range(k):
        for j in range(i + 1, k):
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            out[:, p] = K[:, si] @ coef[j - 1, si] + K[:, sj] @ coef[i, sj] - m["rho"][p]
            p += 1
    return out


def votes_winner(dec, k):
    """svm_predict: a positive decision value votes for i, else j; first maximum wins."""
    votes = np.zeros((dec.shape[0], k), dtype=np.int64)
    p = 0
    for i in range(k):
        for j in range(i + 1, k):
            pos = dec[:, p] > 0
            votes[pos, i] += 1
            votes[~pos, j] += 1
            p += 1
    return np.argmax(votes, axis=1)


def sigmoid_predict(dec, a, b):
    f = dec * a + b
    return np.where(f >= 0, np.exp(-np.abs(f)) / (1.0 + np.exp(-np.abs(f))), 1.0 / (1 + np.exp(np.minimum(f, 0))))


def multiclass_probability(r):
    """libsvm's multiclass_probability for one pairwise matrix r [k][k], operation by operation."""
    k = r.shape[0]
    Q = np.zeros((k, k))
    p = np.full(k, 1.0 / k)
    for t in range(k):
        for j in range(t):
            Q[t, t] += r[j, t] * r[j, t]
            Q[t, j] = Q[j, t]
        for j in range(t + 1, k):
            Q[t, t] += r[j, t] * r[j, t]
            Q[t, j] = -r[j, t] * r[t, j]
    max_iter, eps = max(100, k), 0.005 / k
    Qp = np.zeros(k)
    for _ in range(max_iter):
        pQp = 0.0
        for t in range(k):
            Qp[t] = 0.0
            for j in range(k):
                Qp[t] += Q[t, j] * p[j]
            pQp += p[t] * Qp[t]
        if np.max(np.abs(Qp - pQp)) < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t, j]) / (1 + diff)
                p[j] /= (1 + diff)
    return p


def probabilities(m, dec):
    k = len(m["n_support"])
    out = np.empty((dec.shape[0], k))
    for v in range(dec.shape[0]):
        r = np.zeros((k, k))
        p = 0
        for i in range(k):
            for j in range(i + 1, k):
                r[i, j] = min(max(float(sigmoid_predict(dec[v, p], m["prob_a"][p], m["prob_b"][p])), 1e-7), 1 - 1e-7)
                r[j, i] = 1 - r[i, j]
                p += 1
        out[v] = multiclass_probability(r)
    return out


def predict(m, X):
    """(label index [n_vec], probabilities [n_vec][k], decision values) of standardised vectors X [n_vec][n_dims]."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    dec = decision_values(m, X)
    k = len(m["n_support"])
    return votes_winner(dec, k), probabilities(m, dec), dec


# the class sizes of the two shipped models too large to carry as golden files (pyAudioAnalysis/data/models: 1.1 MB and
# 2.5 MB of float64 support vectors); synthetic_model builds seeded stand-ins of exactly their shape
SPEAKER_10_N_SUPPORT = (111, 97, 104, 93, 100, 113, 105, 109, 97, 92)
MOVIE8CLASS_N_SUPPORT = (256, 358, 252, 174, 148, 330, 409, 346)


def synthetic_model(n_support, n_dims, seed, kernel="rbf"):
    """A model in libsvm's layout with the given class sizes: support vectors ~ N(0, 1), dual coefficients in [-1, 1]
    (|alpha| <= C = 1 as in the shipped models), gamma = 1 / n_dims (scikit-learn's 'auto', the shipped models' value),
    Platt parameters in the shipped models' range -- decision values of both signs and non-degenerate probabilities for
    standardised inputs.  Arithmetic coverage only: it is not a trained classifier."""
    rng = np.random.default_rng(seed)
    ns = np.asarray(n_support, dtype=np.int32)
    k, n_sv = ns.shape[0], int(ns.sum())
    pairs = k * (k - 1) // 2
    return {"support_vectors": rng.standard_normal((n_sv, n_dims)), "n_support": ns,
            "dual_coef": rng.uniform(-1.0, 1.0, (k - 1, n_sv)), "rho": rng.normal(0.0, 0.3, pairs),
            "prob_a": -rng.uniform(2.0, 7.0, pairs), "prob_b": rng.normal(0.0, 0.3, pairs),
            "gamma": 1.0 / n_dims if kernel == "rbf" else 0.0, "kernel": kernel}
