"""NumPy FP64 restatement of the batched epsilon-SVR solver and of the SVR split sweep (pyaudioanalysis_amd/csrc/kernels_svrfit.hpp;
audioTrainTest.svr_solve / svr_split_fit_predict / evaluate_regression(svm_fit="device")) -- the CPU second opinion of the GPU
kernel.  Test helper, not part of the package.

solve() is libsvm's solve_epsilon_svr over its Solver without shrinking (sklearn/svm/src/libsvm/svm.cpp: Solver::Solve,
select_working_set, calculate_rho) on a precomputed n x n Gram matrix, in float64 throughout (libsvm keeps its kernel cache in
float32).  The dual has 2 n variables: variable v stands for row v mod n, its sign is +1 for v < n and -1 for v >= n, its linear
term epsilon - y for v < n and epsilon + y for v >= n, and Q_uv = sign_u sign_v K[u mod n, v mod n]."""
import contextlib

import numpy as np

from smo_ref import STATUS_CONVERGED, STATUS_NOT_CONVERGED, TAU, gap_and_sets, gram, rho_of

SVR_EPSILON = 0.1           # scikit-learn's default, which train_svm_regression leaves in place


def dual_signs(n):
    return np.concatenate([np.ones(n), -np.ones(n)])


MUTANTS = ("least_index", "first_order", "swapped_clips", "no_second_clip", "no_tau")
STATUS_NOT_FINITE = -1      # a mutant's run that left the numbers (no status of the library)


def _margin_and_partner(values, candidates, chosen, n):
    """(the chosen candidate's value minus the best value of a candidate that is neither it nor the other variable of its row:
    inf when there is none, 0 for an exact tie; the chosen value minus that other variable's, inf when it is no candidate)."""
    partner = chosen + n if chosen < n else chosen - n
    others = candidates.copy()
    others[chosen] = others[partner] = False
    margin = float(values[chosen] - np.max(values[others])) if others.any() else np.inf
    return margin, float(values[chosen] - values[partner]) if candidates[partner] else np.inf


def solve(K, targets, C, epsilon=SVR_EPSILON, eps=1e-3, max_iter=10**7, trace=None, mutant=None):
    """(alpha [2 n], G [2 n], rho, iterations, gap, status) of min 1/2 a^T Q a + p^T a, 0 <= a <= C, s^T a = 0.
    trace: a list that receives one dict per iteration -- i, j (variables, 0 .. 2 n - 1); branches, the clips of the update that
    fired (A1..A4 for s_i != s_j, B1..B4 for equal signs, in the order of the ifs below, as smo_ref.solve names them); tau,
    whether eta of the chosen pair was not positive; eta_rel = eta / (QD_i + QD_j); g_scale = max(1, max |G|) and gap =
    Gmax + Gmax2 of the state the iteration started from; margin_i / margin_j, the chosen candidate's value (v over I_up; b^2 /
    eta over the candidates of j) minus the best value of a candidate that is NOT the other variable of the same row; partner_i /
    partner_j, the chosen value minus that other variable's (inf: it was no candidate), and row_tie_i / row_tie_j, whether that is
    exactly 0 (at epsilon = 0 G[t + n] == -G[t] holds bit for bit, so it always is when both are candidates; the greatest index,
    t + n, is chosen); both_above, whether the state the iteration started from holds both alphas of some row above zero;
    clip_margin, the least distance, in units of C, of one of the two new values BEFORE the clips from one of the bounds 0 and C:
    what decides whether a clip fires; bound_margin, the least distance, in units of C, of a new value AFTER the clips from a
    bound, over the new values that are not 0 or C in any arithmetic (those are: the value a clip assigns, and the other value of
    a clipped step whose two old values were such): a value that meets a bound only because two roundings agree -- alpha_i -
    alpha_j = 0 for two variables that have moved together -- is at the bound for this solver and one ulp inside it for another,
    where it remains a candidate.
    mutant: a solver that breaks one rule (tests/test_svr_edges_ref_cpu.py shows that the GPU test tells each from this one) --
    "least_index": ties go to the least index; "first_order": j is the candidate of the greatest b, not of the greatest b^2 /
    eta; "swapped_clips": the second clip pass of a branch runs before the first; "no_second_clip": it does not run at all;
    "no_tau": an eta <= 0 is left as it is (a run that leaves the finite numbers stops with STATUS_NOT_FINITE)."""
    assert mutant is None or mutant in MUTANTS, mutant
    t = np.asarray(targets, dtype=np.float64)
    n = t.shape[0]
    s = dual_signs(n)
    alpha, G = np.zeros(2 * n), np.concatenate([epsilon - t, epsilon + t])
    QD = np.concatenate([np.diagonal(K), np.diagonal(K)])
    it, idx = 0, np.arange(2 * n)
    exact = np.ones(2 * n, dtype=bool)                  # for the trace: alpha_v is 0 or C in ANY arithmetic (see bound_margin)
    while True:
        gmax, gmax2, up, low, v = gap_and_sets(alpha, G, s, C)
        if mutant is not None and not (np.all(np.isfinite(alpha)) and np.all(np.isfinite(G))):
            status = STATUS_NOT_FINITE
            break
        if not up.any() or gmax + gmax2 < eps:
            status = STATUS_CONVERGED
            break
        if it >= max_iter:
            status = STATUS_NOT_CONVERGED
            break
        cand_i = idx[up]
        vi = v[up]
        i = int(cand_i[vi.shape[0] - 1 - int(np.argmax(vi[::-1]))])       # the greatest index attaining the maximum
        if mutant == "least_index":
            i = int(cand_i[int(np.argmax(vi))])
        Ki = np.concatenate([K[i % n], K[i % n]])
        b = gmax - v
        cand = low & (b > 0)
        if not cand.any():
            status = STATUS_CONVERGED
            break
        eta = QD[i] + QD - 2.0 * Ki
        if mutant != "no_tau":
            eta = np.where(eta > 0, eta, TAU)
        if mutant == "first_order":
            obj = np.where(cand, -b, np.inf)
        elif mutant == "no_tau":
            with np.errstate(all="ignore"):
                obj = np.where(cand, -(b * b) / eta, np.inf)
            obj = np.where(np.isnan(obj), np.inf, obj)
        else:
            obj = np.where(cand, -(b * b) / eta, np.inf)
        j = 2 * n - 1 - int(np.argmin(obj[::-1]))
        if mutant == "least_index":
            j = int(np.argmin(obj))
        ai, aj = alpha[i], alpha[j]
        fired = []
        with np.errstate(all="ignore") if mutant == "no_tau" else contextlib.nullcontext():
            if s[i] != s[j]:
                delta = (-G[i] - G[j]) / eta[j]
                d = ai - aj
                ni, nj = ai + delta, aj + delta
                raw = (ni, nj)
                for first in ((False, True) if mutant == "swapped_clips" else (True,) if mutant == "no_second_clip" else (True, False)):
                    if first:
                        if d > 0 and nj < 0:
                            nj, ni = 0.0, d
                            fired.append("A1")
                        elif d <= 0 and ni < 0:
                            ni, nj = 0.0, -d
                            fired.append("A2")
                    else:
                        if d > 0 and ni > C:
                            ni, nj = C, C - d
                            fired.append("A3")
                        elif d <= 0 and nj > C:
                            nj, ni = C, C + d
                            fired.append("A4")
            else:
                delta = (G[i] - G[j]) / eta[j]
                sm = ai + aj
                ni, nj = ai - delta, aj + delta
                raw = (ni, nj)
                for first in ((False, True) if mutant == "swapped_clips" else (True,) if mutant == "no_second_clip" else (True, False)):
                    if first:
                        if sm > C and ni > C:
                            ni, nj = C, sm - C
                            fired.append("B1")
                        elif sm <= C and nj < 0:
                            nj, ni = 0.0, sm
                            fired.append("B2")
                    else:
                        if sm > C and nj > C:
                            nj, ni = C, sm - C
                            fired.append("B3")
                        elif sm <= C and ni < 0:
                            ni, nj = 0.0, sm
                            fired.append("B4")
            if trace is not None:
                eta_raw = QD[i] + QD[j] - 2.0 * Ki[j]
                literal = {"A1": j, "A2": i, "A3": i, "A4": j, "B1": i, "B2": j, "B3": j, "B4": i}
                sure = exact[i] and exact[j] and bool(fired)        # d, sm and what a clip forms of them: sums of 0 and C
                exact[i], exact[j] = (sure or any(literal[b] == i for b in fired)), (sure or any(literal[b] == j for b in fired))
                loose = [a for a, e in ((ni, exact[i]), (nj, exact[j])) if not e]
                bound_margin = float(min(min(abs(a), abs(C - a)) for a in loose) / C) if loose else np.inf
                margin_i, partner_i = _margin_and_partner(v, up, i, n)
                margin_j, partner_j = _margin_and_partner(-obj, cand, j, n)
                trace.append(dict(i=i, j=j, branches=tuple(fired), tau=not eta_raw > 0, bound_margin=bound_margin,
                                  clip_margin=float(min(abs(r - bound) for r in raw for bound in (0.0, C)) / C),
                                  eta_rel=float(eta[j] / (QD[i] + QD[j])) if QD[i] + QD[j] > 0 else np.inf,
                                  g_scale=float(max(1.0, np.max(np.abs(G)))), gap=float(gmax + gmax2), margin_i=margin_i, margin_j=margin_j,
                                  partner_i=partner_i, partner_j=partner_j, row_tie_i=partner_i == 0.0, row_tie_j=partner_j == 0.0,
                                  both_above=bool(np.any((alpha[:n] > 0) & (alpha[n:] > 0)))))
            Kj = np.concatenate([K[j % n], K[j % n]])
            G += s * (Ki * (s[i] * (ni - ai)) + Kj * (s[j] * (nj - aj)))
        alpha[i], alpha[j] = ni, nj
        it += 1
    gap = gmax + gmax2 if np.isfinite(gmax) and np.isfinite(gmax2) else 0.0
    return alpha, G, rho_of(alpha, G, s, C), it, float(gap), status


def solve_trace(K, targets, C, epsilon=SVR_EPSILON, eps=1e-3, max_iter=10**7, mutant=None):
    """solve() and the list of its iterations (see solve)."""
    trace = []
    return solve(K, targets, C, epsilon, eps, max_iter, trace, mutant), trace


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
