"""NumPy restatement of the LDA branch of pyAudioAnalysis's speaker_diarization (audioSegmentation.py:880-934): scikit-learn's
LinearDiscriminantAnalysis(n_components, solver="svd", tol=1e-4).fit_transform with empirical priors -- the CPU second
opinion for pyaudioanalysis_amd/csrc/kernels_lda.hpp and audioSegmentation.lda_fit_device.  Test helper, not part of the
package.  It takes TRUE singular value decompositions (numpy.linalg.svd), where the package goes through the Gram matrices
and numpy.linalg.eigh: the two routes share no decomposition.

Steps (X = n windows x D, labels non-decreasing, C classes):

  m_c class means, p_c = n_c / n, xbar = sum p_c m_c;  Xc = X - m_label;  std = Xc.std(axis = 0), exact zeros -> 1
  S, V of sqrt(1 / (n - C)) Xc / std;  rank = #{S > tol};  scalings = (V[:rank] / std).T / S[:rank]
  S2, V2 of (sqrt(n p_c / (C - 1)) (m_c - xbar).T).T @ scalings;  rank2 = #{S2 > tol S2[0]};  scalings_ = scalings @ V2.T[:, :rank2]
  SIGN RULE (an SVD leaves it open): every column of scalings_ has its largest-magnitude entry positive
  Y = (X - xbar) @ scalings_[:, :n_components]

MARGINS say how far every decision is from flipping: rank_margin = (min kept S / tol, tol / max dropped S), rank2_margin the
same against tol S2[0]; s2_gap the smallest relative gap between consecutive S2 among the kept ones that matter (the first
n_components and their successor): the singular vectors of close values are not determined; sign_margin = 1 - the largest
ratio second-largest |entry| / largest |entry| over the columns in use."""
import numpy as np

TOL = 1e-4


def window_labels(n_windows, short_window):
    """The reference's loop (:925-929), as written."""
    labels = np.zeros((n_windows,))
    lda_step = 1.0
    lda_step_ratio = lda_step / short_window
    for index in range(labels.shape[0]):
        labels[index] = int(index * short_window / lda_step_ratio)
    return labels.astype(np.int64)


def run_offsets(labels):
    labels = np.asarray(labels)
    starts = np.flatnonzero(np.concatenate(([True], labels[1:] != labels[:-1])))
    return np.concatenate((starts, [labels.shape[0]])).astype(np.int64)


def sign_fix(M):
    """(M with every column's largest-magnitude entry positive, the flips [columns] as +-1, sign_margin)."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape[1] == 0:
        return M.copy(), np.ones(0), np.inf
    mag = np.abs(M)
    top = np.argmax(mag, axis=0)
    flips = np.where(M[top, np.arange(M.shape[1])] < 0, -1.0, 1.0)
    if M.shape[0] > 1:
        two = np.sort(mag, axis=0)[-2:]
        margin = float(1.0 - np.max(two[0] / two[1]))
    else:
        margin = np.inf
    return M * flips, flips, margin


def _margins(S, rank, threshold):
    kept = float(S[rank - 1] / threshold) if rank > 0 else 0.0
    dropped = float(threshold / S[rank]) if rank < S.shape[0] and S[rank] > 0 else np.inf
    return kept, dropped


def class_stats(X, labels):
    """(means [C][D], std [D] with zeros replaced by 1, offsets) -- means first, then deviations."""
    X = np.asarray(X, dtype=np.float64)
    off = run_offsets(labels)
    C = off.shape[0] - 1
    means = np.stack([X[off[c]:off[c + 1]].mean(axis=0) for c in range(C)])
    Xc = X - np.repeat(means, np.diff(off), axis=0)
    std = Xc.std(axis=0)
    std[std == 0] = 1.0
    return means, std, off


def fit(X, labels, n_components, tol=TOL):
    """dict: means, std, priors, xbar, gram (of the scaled centred matrix), S, rank, S2, rank2, scalings (sign-fixed, first
    n_components columns), Y, and the margins."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    means, std, off = class_stats(X, labels)
    C = off.shape[0] - 1
    if n_components > min(D, C - 1):
        raise ValueError("n_components cannot be larger than min(n_features, n_classes - 1).")
    if n <= C:
        raise ValueError("The number of samples must be more than the number of classes.")
    priors = np.diff(off) / float(n)
    xbar = priors @ means
    Xc = X - np.repeat(means, np.diff(off), axis=0)
    Xs = np.sqrt(1.0 / (n - C)) * (Xc / std)
    _, S, Vt = np.linalg.svd(Xs, full_matrices=False)
    rank = int(np.sum(S > tol))
    scalings = (Vt[:rank] / std).T / S[:rank]
    fac = 1.0 if C == 1 else 1.0 / (C - 1)
    W = ((np.sqrt((n * priors) * fac)) * (means - xbar).T).T @ scalings
    _, S2, Vt2 = np.linalg.svd(W, full_matrices=False)
    rank2 = int(np.sum(S2 > tol * S2[0]))
    full, _, _ = sign_fix(scalings @ Vt2.T[:, :rank2])
    used = full[:, :n_components]
    _, _, sign_margin = sign_fix(used)
    upto = min(n_components + 1, rank2)
    gaps = (S2[:upto - 1] - S2[1:upto]) / S2[:upto - 1] if upto > 1 else np.array([np.inf])
    return {"means": means, "std": std, "priors": priors, "xbar": xbar, "offsets": off, "gram": Xs.T @ Xs, "S": S, "rank": rank,
            "S2": S2, "rank2": rank2, "scalings": used, "Y": (X - xbar) @ used,
            "rank_margin": _margins(S, rank, tol), "rank2_margin": _margins(S2, rank2, tol * S2[0]),
            "s2_gap": float(np.min(gaps)), "sign_margin": sign_margin}


def planted(seed, n, d, runs, spread=3.0, speakers=4):
    """(X [n][d], labels [n]): windows around `speakers` planted means, the speaker changing from run to run; `runs` the run
    lengths (their sum is n)."""
    rng = np.random.default_rng(seed)
    assert sum(runs) == n
    centres = rng.standard_normal((speakers, d)) * spread
    who = np.concatenate([np.full(r, rng.integers(speakers)) for r in runs])
    labels = np.concatenate([np.full(r, c) for c, r in enumerate(runs)]).astype(np.int64)
    X = centres[who] + rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, d)
    return X, labels


def equal_runs(n, C):
    """C run lengths that add up to n: the first ones one longer, so the last run is a short one when C does not divide n."""
    base, extra = divmod(n, C)
    return [base + 1] * extra + [base] * (C - extra)


def edge_cases():
    """[(id, X [n][D], labels, n_components)]: the smallest shapes at which the kernels can go wrong -- D = 1, 2, 3, 17, 148, 256;
    n = C + 1, 63, 64, 65, 1000; C = 2 (one output column); C - 1 below and above D; runs of a single window, a short last run;
    a constant dimension; a duplicated dimension and a block of rows that sums to a constant (both rank-deficient);
    n_components 1 and min(D, C - 1)."""
    out = []
    X, y = planted(1, 63, 1, equal_runs(63, 3), speakers=3)
    out.append(("d1_n63_c3", X, y, 1))
    X, y = planted(2, 64, 2, equal_runs(64, 2), speakers=2)
    out.append(("d2_n64_c2", X, y, 1))
    X, y = planted(3, 6, 3, [2, 1, 1, 1, 1], speakers=3)
    out.append(("d3_n6_c5", X, y, 1))
    X, y = planted(4, 63, 3, equal_runs(63, 8), speakers=4)
    out.append(("d3_n63_c8", X, y, 3))
    X, y = planted(5, 65, 17, [20, 1, 13, 17, 11, 3], speakers=3)
    out.append(("d17_n65_c6", X, y, 5))
    X, y = planted(6, 1000, 148, equal_runs(1000, 40), speakers=6)
    X[:, 100] = 2.5
    out.append(("d148_n1000_c40_const", X, y, 35))
    X, y = planted(7, 1000, 256, equal_runs(1000, 40), speakers=5)
    out.append(("d256_n1000_c40", X, y, 1))
    X, y = planted(8, 200, 10, equal_runs(200, 8), speakers=4)
    X[:, 7] = X[:, 2]
    out.append(("d10_duplicate", X, y, 3))
    X, y = planted(9, 200, 12, equal_runs(200, 8), speakers=4)
    e = np.exp(X[:, 4:8] * 0.3)
    X[:, 4:8] = e / e.sum(axis=1, keepdims=True)
    out.append(("d12_rows_sum_to_one", X, y, 3))
    return [(name, np.ascontiguousarray(X), y, nc) for name, X, y, nc in out]


def synthetic_speaker_models():
    """Seeded SVMs of the shipped shapes (10 speakers, male / female) as load_model tuples."""
    import svc_libsvm
    from pyaudioanalysis_amd import audioTrainTest
    out = []
    for n_classes, seed in ((10, 1), (2, 2)):
        m = svc_libsvm.synthetic_model([4] * n_classes, 136, seed)
        clf = audioTrainTest.SvcArrays(m["support_vectors"], m["n_support"], m["dual_coef"], -m["rho"], m["prob_a"], m["prob_b"],
                                       m["gamma"], "rbf", np.arange(n_classes, dtype=np.float64))
        rng = np.random.default_rng(seed)
        out.append((clf, rng.standard_normal(136) * 0.1, 0.5 + rng.random(136), ["c%d" % i for i in range(n_classes)], 1.0, 0.1,
                    0.05, 0.05, False))
    return out
