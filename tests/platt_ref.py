"""NumPy FP64 restatement of the second half of libsvm's probability=True (pyaudioanalysis_amd/csrc/kernels_platt.hpp and the
fold construction of lib_smo.hpp; audioTrainTest.platt_sigmoid / svc_fit_proba) -- the CPU second opinion of the GPU path.
Test helper, not part of the package.

sigmoid_train() is svm.cpp's sigmoid_train operation for operation, with the sums in NumPy's order.  pair_folds() builds
svm_binary_svc_probability's five folds of a class pair from libsvm's random_seed: std::mt19937(seed) (its raw 32-bit outputs
are those of np.random.RandomState(seed)), restarted for every pair; the bounded draw of scikit-learn's newrand.h (Lemire's
method with rejection); perm shuffled by j = i + bounded(l - i), swap(perm[i], perm[j]); fold f holds out
perm[f l // 5 : (f + 1) l // 5].  fit() is the whole fit of a job with smo_ref.solve / smo_ref.gram for the tasks, or with any
other fold solver (scikit-learn's probability=False fits in the CPU test)."""
import numpy as np

import smo_ref

STOP_CONVERGED, STOP_LINE_SEARCH_FAILED, STOP_MAX_ITERATIONS = 0, 1, 2
MAX_ITER, MIN_STEP, SIGMA, EPS = 100, 1e-10, 1e-12, 1e-5
NOISE = 1e9 * np.finfo(np.float64).eps       # see sigmoid_train: the line-search margin's floor, in units of max(1, |fval|)


def _objective(dec, t, A, B):
    with np.errstate(over="ignore", invalid="ignore"):
        f = dec * A + B
        return float(np.sum(np.where(f >= 0, t * f + np.log(1 + np.exp(-f)), (t - 1) * f + np.log(1 + np.exp(f)))))


def sigmoid_train(dec, signs):
    """(A, B, iterations, stop, margin) of libsvm's sigmoid_train on the decision values dec with the signs (+1: the first class).
    margin: the smallest margin met at any decision of the run --
      the stop test |g1| < 1e-5 and |g2| < 1e-5: ||g| - 1e-5| / 1e-5, the smaller of the two when the test holds, the greatest
      over the components that break it when it does not;
      every line-search test newf < fval + 1e-4 step gd: |newf - (fval + 1e-4 step gd)| / max(step |gd|, NOISE max(1, |fval|)),
      the distance in units of the predicted decrease, but never in units finer than 1e9 roundings of the objective -- a
      different order of the sums moves newf by a few roundings.
    A test on a value that is not finite (a decision value was infinite or NaN) has no margin: a comparison with a NaN is false
    under any rounding."""
    dec = np.asarray(dec, dtype=np.float64)
    pos = np.asarray(signs) > 0
    prior1, prior0 = float(np.count_nonzero(pos)), float(np.count_nonzero(~pos))
    t = np.where(pos, (prior1 + 1.0) / (prior1 + 2.0), 1.0 / (prior0 + 2.0))
    A, B = 0.0, float(np.log((prior0 + 1.0) / (prior1 + 1.0)))
    fval = _objective(dec, t, A, B)
    margin, stop, it = np.inf, STOP_MAX_ITERATIONS, 0
    for it in range(MAX_ITER + 1):
        if it == MAX_ITER:
            break
        with np.errstate(over="ignore", invalid="ignore"):
            f = dec * A + B
            p = np.where(f >= 0, np.exp(-f) / (1.0 + np.exp(-f)), 1.0 / (1.0 + np.exp(f)))
            q = np.where(f >= 0, 1.0 / (1.0 + np.exp(-f)), np.exp(f) / (1.0 + np.exp(f)))
        d2, d1 = p * q, t - p
        h11 = SIGMA + float(np.sum(dec * dec * d2))
        h22 = SIGMA + float(np.sum(d2))
        h21 = float(np.sum(dec * d2))
        g1, g2 = float(np.sum(dec * d1)), float(np.sum(d1))
        m = [abs(abs(g) - EPS) / EPS for g in (g1, g2)]
        if abs(g1) < EPS and abs(g2) < EPS:
            margin = min(margin, m[0], m[1])
            stop = STOP_CONVERGED
            break
        if np.isfinite(g1) and np.isfinite(g2):
            margin = min(margin, max(mi for mi, g in zip(m, (g1, g2)) if not abs(g) < EPS))
        with np.errstate(all="ignore"):
            det = np.float64(h11) * h22 - np.float64(h21) * h21
            dA = float(-(h22 * g1 - h21 * g2) / det)
            dB = float(-(-h21 * g1 + h11 * g2) / det)
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= MIN_STEP:
            newA, newB = A + step * dA, B + step * dB
            newf = _objective(dec, t, newA, newB)
            rhs = fval + 0.0001 * step * gd
            if np.isfinite(newf) and np.isfinite(rhs):      # (a comparison with a NaN is false under any rounding)
                margin = min(margin, abs(newf - rhs) / max(step * abs(gd), NOISE * max(1.0, abs(fval))))
            if newf < rhs:
                A, B, fval = newA, newB, newf
                break
            step = step / 2.0
        if step < MIN_STEP:
            stop = STOP_LINE_SEARCH_FAILED
            break
    return A, B, it, stop, float(margin)


class _Mt:
    """std::mt19937(seed)'s raw outputs and libsvm's bounded draw over them."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(int(seed))

    def raw(self):
        return int.from_bytes(self.rs.bytes(4), "little")

    def bounded(self, rng):
        m = self.raw() * rng
        low = m & 0xffffffff
        if low < rng:
            t = (2**32 - rng) % rng
            while low < t:
                m = self.raw() * rng
                low = m & 0xffffffff
        return m >> 32


def permutation(l, seed):
    """svm_binary_svc_probability's perm of l rows for libsvm's random_seed."""
    gen = _Mt(seed)
    perm = list(range(l))
    for i in range(l):
        j = i + gen.bounded(l - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm, dtype=np.int64)


def pair_folds(signs, seed):
    """The five folds of a pair whose rows, in pair-row order, have the signs `signs`: a list of (held, train, constant) --
    held: the held-out positions in permutation order; train: the training positions in libsvm's sub-problem order
    (permutation order, grouped by class, the class seen first put first), or None for a fold that makes no fit, whose held-out
    decision values are then `constant` (+1: only the first class trains, -1: only the second, 0: neither)."""
    signs = np.asarray(signs)
    l = signs.shape[0]
    perm = permutation(l, seed)
    folds = []
    for f in range(5):
        begin, end = f * l // 5, (f + 1) * l // 5
        held, rest = perm[begin:end], np.concatenate([perm[:begin], perm[end:]])
        sg = signs[rest]
        if rest.shape[0] == 0 or (sg == sg[0]).all():
            folds.append((held, None, 0.0 if rest.shape[0] == 0 else float(np.sign(sg[0]))))
            continue
        folds.append((held, np.concatenate([rest[sg == sg[0]], rest[sg != sg[0]]]), None))
    return folds


def solve_fold(Z, y, C, kernel, gamma, eps, Zq):
    """The restatement's fit of the rows Z with the signs y and its decision values of the rows Zq:
    (dec, alpha_y, rho, iterations, status)."""
    alpha, rho, it, _, st = smo_ref.solve(smo_ref.gram(Z, kernel, gamma), y, float(C), eps)
    sv = alpha != 0
    dec = smo_ref.gram(Zq, kernel, gamma, Z[sv]) @ (alpha * y)[sv] - rho if Zq.shape[0] else np.zeros(0)
    return dec, alpha * y, rho, it, st


def fit(X, labels, job, seed, kernel="linear", gamma=None, eps=1e-3, fold_dec=None):
    """SVC(probability=True).fit of one job (train_idx, mean, scale, C) for libsvm's random_seed: per pair (a, b), a < b, of the
    classes present a dict with rows (sample indices in pair-row order), signs, alpha_y, rho, n_sv, iterations / status [6]
    (slot 0: the full fit, 1..5: the folds, 0 for a fold without a fit), cv_dec, degenerate (the rows whose cv_dec is a
    constant), prob_a, prob_b, sigmoid_iterations, sigmoid_stop, sigmoid_margin.  Returns (classes, [pair dicts]).
    fold_dec(Z, y, C, Zq) -> held-out decision values, positive for sign +1, replaces the restatement's fold fits."""
    train_idx, mean, scale, C = job
    X = np.asarray(X, dtype=np.float64)
    gamma = 1.0 / X.shape[1] if gamma is None else gamma
    classes, tasks = smo_ref.pair_tasks(labels, train_idx)
    pairs = []
    for a, b, rows, y in tasks:
        Z = (X[rows] - mean) / scale
        _, alpha_y, rho, it, st = solve_fold(Z, y, C, kernel, gamma, eps, Z[:0])
        its, status = [it], [st]
        cv, degenerate = np.zeros(rows.shape[0]), np.zeros(rows.shape[0], dtype=bool)
        for held, train, constant in pair_folds(y, seed):
            if train is None:
                cv[held], degenerate[held] = constant, True
                its.append(0)
                status.append(0)
                continue
            if fold_dec is not None:
                cv[held] = fold_dec(Z[train], y[train], C, Z[held]) if held.shape[0] else np.zeros(0)
                its.append(-1)
                status.append(-1)
                continue
            dec, _, _, it, st = solve_fold(Z[train], y[train], C, kernel, gamma, eps, Z[held])
            cv[held] = dec
            its.append(it)
            status.append(st)
        A, B, sit, stop, margin = sigmoid_train(cv, y)
        pairs.append(dict(a=a, b=b, rows=rows, signs=y, alpha_y=alpha_y, rho=rho, n_sv=int(np.count_nonzero(alpha_y)),
                          iterations=np.array(its), status=np.array(status), cv_dec=cv, degenerate=degenerate, prob_a=A, prob_b=B,
                          sigmoid_iterations=sit, sigmoid_stop=stop, sigmoid_margin=margin))
    return classes, pairs


class Model:
    """A fitted probabilistic SVC as arrays in scikit-learn's attribute names (what audioTrainTest.to_sklearn_svc, svc_model and
    audioSegmentation.svm_onset_probability read)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def model_of(X, labels, job, classes, pairs, kernel, gamma=None):
    """libsvm's model of a fit() result: the support vectors are the union over the pairs, grouped by class ascending, in
    train-list order within a class; _dual_coef_ [k - 1][n_SV]: for the pair (a, b) class a's coefficients in row b - 1,
    class b's in row a; _intercept_ = -rho; the public dual_coef_ / intercept_ negated for two classes."""
    train_idx, mean, scale, C = job
    X = np.asarray(X, dtype=np.float64)
    train_idx = np.asarray(train_idx, dtype=np.int64)
    k = len(classes)
    cls = np.searchsorted(classes, np.asarray(labels)[train_idx])
    place = {int(s): i for i, s in enumerate(train_idx)}
    coef = np.zeros((k - 1, len(train_idx)))
    for q in pairs:
        for s, ay, sg in zip(q["rows"], q["alpha_y"], q["signs"]):
            coef[q["b"] - 1 if sg > 0 else q["a"], place[int(s)]] = ay
    sv = np.flatnonzero(np.any(coef != 0, axis=0))
    sv = sv[np.argsort(cls[sv], kind="stable")]
    flip = -1.0 if k == 2 else 1.0
    dual, icpt = coef[:, sv], -np.array([q["rho"] for q in pairs])
    n_support = np.bincount(cls[sv], minlength=k).astype(np.int32)
    return Model(support_=sv.astype(np.int32), support_vectors_=(X[train_idx[sv]] - mean) / scale, n_support_=n_support, _n_support=n_support,
                 _dual_coef_=dual, dual_coef_=flip * dual, _intercept_=icpt, intercept_=flip * icpt,
                 probA_=np.array([q["prob_a"] for q in pairs]), probB_=np.array([q["prob_b"] for q in pairs]), classes_=np.asarray(classes),
                 kernel=kernel, _gamma=1.0 / X.shape[1] if gamma is None else gamma, C=float(C), shape_fit_=(len(train_idx), X.shape[1]))
