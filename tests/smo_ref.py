"""NumPy FP64 restatement of the batched SMO solver and the one-against-one scoring of the SVM split sweep
(pyaudioanalysis_amd/csrc/kernels_smo.hpp; audioTrainTest.svm_split_fit_predict / smo_solve) -- the CPU second opinion of the
GPU kernels.  Test helper, not part of the package.

solve() is libsvm's Solver for C-SVC without shrinking (sklearn/svm/src/libsvm/svm.cpp: Solver::Solve, select_working_set,
calculate_rho) on a precomputed Gram matrix, in float64 throughout (libsvm keeps its kernel cache in float32).  A task is a
list of rows, a sign per row (+1: the first class of the pair), C and eps; fit_job() builds the pair tasks of a split as the
library does: the classes PRESENT in the training list in ascending order, per pair the rows of the first class in
train-list order, then those of the second."""
import warnings

import numpy as np

TAU = 1e-12
STATUS_CONVERGED, STATUS_NOT_CONVERGED = 2, 3
KERNEL_TYPES = {"linear": 0, "rbf": 2}


def gram(Z, kernel, gamma, W=None):
    """K[a, b] of the standardised rows Z [n][d] against W [m][d] (W = None: Z); RBF in the difference form."""
    W = Z if W is None else W
    if kernel == "linear":
        return Z @ W.T
    d2 = np.empty((Z.shape[0], W.shape[0]))
    for a in range(Z.shape[0]):
        diff = W - Z[a]
        d2[a] = np.einsum("sd,sd->s", diff, diff)
    return np.exp(-gamma * d2)


def _last_argmax(v):
    """The largest index attaining the maximum of v."""
    return v.shape[0] - 1 - int(np.argmax(v[::-1]))


def gap_and_sets(alpha, G, y, C):
    """(Gmax, Gmax2, I_up, I_low, v) of a state: v = -y G, Gmax over I_up, Gmax2 = max of -v over I_low (-inf when empty)."""
    up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < C))
    v = -y * G
    gmax = np.max(v[up]) if up.any() else -np.inf
    gmax2 = np.max(-v[low]) if low.any() else -np.inf
    return gmax, gmax2, up, low, v


def rho_of(alpha, G, y, C):
    """calculate_rho: the mean of y G over the free rows, the midpoint of ub and lb when there is none."""
    yG = y * G
    free = (alpha > 0) & (alpha < C)
    if free.any():
        return float(np.sum(yG[free]) / np.count_nonzero(free))
    upper, lower = alpha >= C, alpha <= 0
    ub_set = (upper & (y < 0)) | (lower & (y > 0))
    lb_set = (upper & (y > 0)) | (lower & (y < 0))
    ub = np.min(yG[ub_set]) if ub_set.any() else np.inf
    lb = np.max(yG[lb_set]) if lb_set.any() else -np.inf
    return float((ub + lb) / 2)


def _margin(values):
    """Best minus second-best of the candidate values of a selection: inf with one candidate, 0 for an exact tie."""
    if values.shape[0] < 2:
        return np.inf
    top = np.partition(values, values.shape[0] - 2)[-2:]
    return float(top[1] - top[0])


def solve(K, y, C, eps=1e-3, max_iter=10**7, trace=None):
    """(alpha, rho, iterations, gap, status) of min 1/2 a^T Q a - e^T a, 0 <= a <= C, y^T a = 0, Q = y y^T K.
    trace: a list that receives one dict per iteration -- i, j; margin_i / margin_j, best minus second-best candidate value of
    the two selections (v over I_up; b^2 / eta over the candidates of j); branches, the clips of the update that fired (A1..A4
    for y_i != y_j, B1..B4 for equal signs, in the order of the ifs below: at most one of each if / elif pair); tau, whether
    eta of the chosen pair was not positive; eta_rel = eta / (QD_i + QD_j); g_scale = max(1, max |G|) and gap = Gmax + Gmax2
    of the state the iteration started from."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    alpha, G, QD = np.zeros(n), -np.ones(n), np.diagonal(K).copy()
    it, idx = 0, np.arange(n)
    while True:
        gmax, gmax2, up, low, v = gap_and_sets(alpha, G, y, C)
        if not up.any() or gmax + gmax2 < eps:
            status = STATUS_CONVERGED
            break
        if it >= max_iter:
            status = STATUS_NOT_CONVERGED
            break
        i = int(idx[up][_last_argmax(v[up])])
        b = gmax - v
        cand = low & (b > 0)
        if not cand.any():
            status = STATUS_CONVERGED
            break
        eta = QD[i] + QD - 2.0 * K[i]
        eta = np.where(eta > 0, eta, TAU)
        obj = np.where(cand, -(b * b) / eta, np.inf)
        j = n - 1 - int(np.argmin(obj[::-1]))
        ai, aj = alpha[i], alpha[j]
        fired = []
        if y[i] != y[j]:
            delta = (-G[i] - G[j]) / eta[j]
            d = ai - aj
            ni, nj = ai + delta, aj + delta
            if d > 0 and nj < 0:
                nj, ni = 0.0, d
                fired.append("A1")
            elif d <= 0 and ni < 0:
                ni, nj = 0.0, -d
                fired.append("A2")
            if d > 0 and ni > C:
                ni, nj = C, C - d
                fired.append("A3")
            elif d <= 0 and nj > C:
                nj, ni = C, C + d
                fired.append("A4")
        else:
            delta = (G[i] - G[j]) / eta[j]
            s = ai + aj
            ni, nj = ai - delta, aj + delta
            if s > C and ni > C:
                ni, nj = C, s - C
                fired.append("B1")
            elif s <= C and nj < 0:
                nj, ni = 0.0, s
                fired.append("B2")
            if s > C and nj > C:
                nj, ni = C, s - C
                fired.append("B3")
            elif s <= C and ni < 0:
                ni, nj = 0.0, s
                fired.append("B4")
        if trace is not None:
            raw = QD[i] + QD[j] - 2.0 * K[i, j]
            trace.append(dict(i=i, j=j, margin_i=_margin(v[up]), margin_j=_margin(-obj[cand]), branches=tuple(fired), tau=not raw > 0,
                              eta_rel=float(eta[j] / (QD[i] + QD[j])) if QD[i] + QD[j] > 0 else np.inf, g_scale=float(max(1.0, np.max(np.abs(G)))),
                              gap=float(gmax + gmax2)))
        G += y * (y[i] * K[i] * (ni - ai) + y[j] * K[j] * (nj - aj))
        alpha[i], alpha[j] = ni, nj
        it += 1
    gap = gmax + gmax2 if np.isfinite(gmax) and np.isfinite(gmax2) else 0.0
    return alpha, rho_of(alpha, G, y, C), it, float(gap), status


def solve_trace(K, y, C, eps=1e-3, max_iter=10**7):
    """solve() and the list of its iterations (see solve)."""
    trace = []
    return solve(K, y, C, eps, max_iter, trace), trace


def gradient(K, y, alpha):
    """G = Q alpha - e recomputed from alpha alone."""
    return y * (K @ (y * alpha)) - 1.0


def pair_tasks(labels, train_idx):
    """(classes present, ascending; [(a, b, rows, signs)] per pair a < b of positions in `classes`): rows are sample indices,
    the first class's in train-list order, then the second's."""
    train_idx = np.asarray(train_idx, dtype=np.int64)
    lab = np.asarray(labels)[train_idx]
    classes = np.unique(lab)
    tasks = []
    for a in range(len(classes)):
        for b in range(a + 1, len(classes)):
            ra, rb = train_idx[lab == classes[a]], train_idx[lab == classes[b]]
            tasks.append((a, b, np.concatenate([ra, rb]), np.concatenate([np.ones(len(ra)), -np.ones(len(rb))])))
    return classes, tasks


def votes_winner(dec, k):
    """libsvm's vote over the pairs (a, b), a < b, row-major: dec > 0 votes for a, else b; the first class with the most votes."""
    votes = np.zeros((dec.shape[0], k), dtype=np.int64)
    p = 0
    for a in range(k):
        for b in range(a + 1, k):
            pos = dec[:, p] > 0
            votes[pos, a] += 1
            votes[~pos, b] += 1
            p += 1
    return np.argmax(votes, axis=1)


def fit_job(X, labels, job, kernel="linear", gamma=None, eps=1e-3, max_iter=10**7):
    """One job (train_idx, test_idx, mean, scale, C): (predicted class labels [n_test], decision values [n_test][pairs],
    iterations [pairs], status [pairs], n_sv [pairs], classes)."""
    train_idx, test_idx, mean, scale, C = job
    X = np.asarray(X, dtype=np.float64)
    gamma = 1.0 / X.shape[1] if gamma is None else gamma
    classes, tasks = pair_tasks(labels, train_idx)
    Zq = (X[np.asarray(test_idx, dtype=np.int64)] - mean) / scale
    dec = np.zeros((Zq.shape[0], len(tasks)))
    its, status, n_sv = [], [], []
    for p, (a, b, rows, y) in enumerate(tasks):
        Z = (X[rows] - mean) / scale
        alpha, rho, it, _, st = solve(gram(Z, kernel, gamma), y, float(C), eps, max_iter)
        sv = alpha != 0
        dec[:, p] = gram(Zq, kernel, gamma, Z[sv]) @ (alpha * y)[sv] - rho
        its.append(it)
        status.append(st)
        n_sv.append(int(np.count_nonzero(sv)))
    pred = classes[votes_winner(dec, len(classes))] if Zq.shape[0] else classes[:0]
    return pred, dec, np.array(its), np.array(status), np.array(n_sv), classes


def evaluate_svm_sweep_ref(features, class_names, classifier_name, params, parameter_mode, n_exp, train_percentage=0.90,
                           eps=1e-3):
    """What evaluate_classifier_full(svm_fit="device") computes, on the CPU: every split drawn up front from NumPy's global
    state in parameter-major order (scikit-learn's train_test_split over the indices), a StandardScaler per split, then the
    restatement's fit of every split.  Returns (chosen parameter, confusion matrices, predictions [parameter][experiment],
    splits [parameter][experiment] as (train_idx, test_idx, mean, scale), decision values [parameter][experiment])."""
    import train_ref
    X, y = train_ref.features_to_matrix(features)
    next_split = train_ref.random_split_source(X.shape[0], train_percentage)
    splits = [[next_split(X, p, e) for e in range(n_exp)] for p in range(len(params))]
    kernel = "rbf" if classifier_name == "svm_rbf" else "linear"
    cache, decs = {}, [[None] * n_exp for _ in params]

    def fit(Xs, ys, param):
        return param

    def classify(param, Xs):
        return cache["pred"]

    def listed(Xm, p, e):
        tr, te, mean, scale = splits[p][e]
        pred, decs[p][e] = fit_job(Xm, y, (tr, te, mean, scale, params[p]), kernel, None, eps)[:2]
        cache["pred"] = [float(v) for v in pred]
        return splits[p][e]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        best, cms, preds, _ = train_ref.evaluate(features, class_names, params, parameter_mode, n_exp, listed, fit, classify)
    preds = [[preds[p * n_exp + e] for e in range(n_exp)] for p in range(len(params))]
    return best, cms, preds, splits, decs
