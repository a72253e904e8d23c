"""NumPy restatement of the Gaussian HMM that pyAudioAnalysis's hmm_segmentation decodes with hmmlearn (GaussianHMM with
diagonal covars_, predict = Viterbi) -- the CPU second opinion for the GPU kernels (pyaudioanalysis_amd/csrc/kernels_hmm.hpp).
hmmlearn is not needed.  Test helper, not part of the package.

log-density of window t under state k, in the direct form, with c = covars_ (the reference stores the per-class standard
deviation there, audioSegmentation.py:340):

    B[t, k] = -0.5 (D log 2 pi + sum_d log c[k, d] + sum_d (x[t, d] - mu[k, d])^2 / c[k, d])

Viterbi as hmmlearn's _viterbi: lat[0] = log pi + B[0]; lat[t, j] = max_i (lat[t-1, i] + log A[i, j]) + B[t, j]; the last
state arg max lat[T-1]; s[t] = arg max_i (lat[t, i] + log A[i, s[t+1]]); every arg max takes the lowest index among equal
maxima (np.argmax); log 0 = -inf.  The MARGIN of a decision is the gap between its best and second-best candidate
(inf with one state); margins[t] belongs to the decision that fixed s[t], the final arg max included."""
import numpy as np


def log_likelihood(X, means, covars):
    """B [n_windows][n_states] of X [n_windows][n_dims]."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    means = np.asarray(means, dtype=np.float64)
    covars = np.asarray(covars, dtype=np.float64)
    d = X.shape[1]
    out = np.empty((X.shape[0], means.shape[0]))
    for k in range(means.shape[0]):
        out[:, k] = -0.5 * (d * np.log(2 * np.pi) + np.log(covars[k]).sum() + (((X - means[k]) ** 2) / covars[k]).sum(axis=1))
    return out


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(p, dtype=np.float64))


def _margin(c):
    if c.shape[0] < 2:
        return np.inf
    second, best = np.sort(c)[-2:]
    return 0.0 if best == second else best - second


def viterbi(startprob, transmat, B):
    """(logprob, states [T] int64, margins [T]) of one sequence with frame log-likelihoods B [T][K]."""
    lpi, lA = _log(startprob), _log(transmat)
    T, K = B.shape
    lat = np.empty((T, K))
    lat[0] = lpi + B[0]
    for t in range(1, T):
        lat[t] = (lat[t - 1][:, None] + lA).max(axis=0) + B[t]
    states = np.empty(T, dtype=np.int64)
    margins = np.empty(T)
    states[T - 1] = int(np.argmax(lat[T - 1]))
    margins[T - 1] = _margin(lat[T - 1])
    for t in range(T - 2, -1, -1):
        c = lat[t] + lA[:, states[t + 1]]
        states[t] = int(np.argmax(c))
        margins[t] = _margin(c)
    return float(lat[T - 1, states[T - 1]]), states, margins


def decode(startprob, transmat, means, covars, X, lengths=None):
    """(logprob per sequence, states, margins) of the rows of X cut into sequences of `lengths`."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    B = log_likelihood(X, means, covars)
    lengths = [X.shape[0]] if lengths is None else [int(n) for n in lengths]
    lp, st, mg, pos = [], [], [], 0
    for n in lengths:
        a, b, c = viterbi(startprob, transmat, B[pos:pos + n])
        lp.append(a)
        st.append(b)
        mg.append(c)
        pos += n
    return np.array(lp), np.concatenate(st), np.concatenate(mg)


def train_statistics(features, labels):
    """train_hmm_compute_statistics (audioSegmentation.py:287-344) restated: features [n_dims][n_windows]."""
    labels = np.asarray(labels)
    uniq = np.unique(labels)
    K = len(uniq)
    if features.shape[1] < labels.shape[0]:
        labels = labels[:features.shape[1]]
    counts = np.array([np.count_nonzero(labels == u) for u in uniq], dtype=np.float64)
    priors = counts / counts.sum()
    trans = np.zeros((K, K))
    for i in range(labels.shape[0] - 1):
        trans[int(labels[i]), int(labels[i + 1])] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(K):
            trans[i] /= trans[i].sum()
    means = np.stack([features[:, labels == u].mean(axis=1) for u in uniq])
    cov = np.stack([features[:, labels == u].std(axis=1) for u in uniq])
    return priors, trans, means, cov


def synthetic_model(K, D, seed, zeros=False):
    """A seeded model whose states are well apart (decisions far from ties): means spread by about 1.5 covars."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((K, D)) * 1.5
    covars = 0.5 + rng.random((K, D))
    trans = rng.random((K, K)) + 4.0 * np.eye(K)
    start = rng.random(K) + 0.1
    if zeros and K > 2:
        trans[0, K - 1] = 0.0
        trans[K - 1, 1] = 0.0
        start[K - 1] = 0.0
    trans /= trans.sum(axis=1, keepdims=True)
    start /= start.sum()
    return start, trans, means, covars


def synthetic_sequence(model, T, seed, dwell=12):
    """T windows drawn from the model's Gaussians along a seeded state path that changes about every `dwell` windows."""
    start, trans, means, covars = model
    rng = np.random.default_rng(seed)
    K, D = means.shape
    path = np.empty(T, dtype=np.int64)
    s = int(rng.integers(K))
    for t in range(T):
        if t and rng.random() < 1.0 / dwell:
            s = int(rng.integers(K))
        path[t] = s
    X = means[path] + np.sqrt(covars[path]) * 0.7 * rng.standard_normal((T, D))
    return X


# ---------------------------------------------------------------------------------------------------------------------
# np.longdouble restatements and designed inputs of the edge suite (tests/test_hmm_edges_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def log_likelihood_ld(X, means, covars):
    """log_likelihood in np.longdouble (the FP64 inputs as they are)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.longdouble))
    means, covars = np.asarray(means, dtype=np.longdouble), np.asarray(covars, dtype=np.longdouble)
    d = X.shape[1]
    out = np.empty((X.shape[0], means.shape[0]), dtype=np.longdouble)
    two_pi = 2 * np.longdouble(np.pi) if np.finfo(np.longdouble).eps == np.finfo(np.float64).eps else \
        np.longdouble(8) * np.arctan(np.longdouble(1))
    with np.errstate(over="ignore"):
        for k in range(means.shape[0]):
            out[:, k] = -0.5 * (d * np.log(two_pi) + np.log(covars[k]).sum() + (((X - means[k]) ** 2) / covars[k]).sum(axis=1))
    return out


def train_statistics_k(features, labels, K, dtype=np.float64):
    """train_statistics for K states given outright (a state that never occurs: prior 0, NaN transition row, means and
    deviations), the sums in `dtype` (np.longdouble: the reference of the tolerance tests)."""
    F = np.asarray(features, dtype=dtype)
    labels = np.asarray(labels).astype(np.int64)[:F.shape[1]]
    counts = np.bincount(labels, minlength=K).astype(np.float64)
    trans = np.zeros((K, K))
    np.add.at(trans, (labels[:-1], labels[1:]), 1.0)
    means, cov = np.full((K, F.shape[0]), np.nan, dtype=dtype), np.full((K, F.shape[0]), np.nan, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        trans = trans / trans.sum(axis=1, keepdims=True)
        for k in range(K):
            sel = F[:, labels == k]
            if sel.shape[1]:
                means[k] = sel.sum(axis=1) / sel.shape[1]
                cov[k] = np.sqrt((((sel - means[k][:, None]) ** 2).sum(axis=1)) / sel.shape[1])
    return counts / counts.sum(), trans, means, cov


def twin_model(K, D, seed, twins=((0, 1),)):
    """synthetic_model in which, for every pair (a, b) of `twins`, state b is a bit-identical copy of state a: same mean,
    covars, start probability, transition row and transition column.  The lattice values of a and b are then bit-equal at
    every step, in any order of summation, and every decision that a wins ties with b."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((K, D)) * 1.5
    covars = 0.5 + rng.random((K, D))
    trans = rng.random((K, K)) + 4.0 * np.eye(K)
    start = rng.random(K) + 0.1
    for a, b in twins:
        means[b], covars[b], start[b] = means[a], covars[a], start[a]
        trans[b, :] = trans[a, :]
        trans[:, b] = trans[:, a]
        trans[a, a] = trans[a, b] = trans[b, a] = trans[b, b] = 2.5     # staying within the pair, either way
    # normalise so that twin rows stay bit-identical: equal rows have equal sums
    trans /= trans.sum(axis=1, keepdims=True)
    start /= start.sum()
    for a, b in twins:
        assert np.array_equal(trans[a], trans[b]) and np.array_equal(trans[:, a], trans[:, b]) and start[a] == start[b]
    return start, trans, means, covars


def higher_twins(twins):
    return sorted(b for _, b in twins)


def viterbi_twins(startprob, transmat, B, twins):
    """viterbi with a third output: the margins of the same decisions with the higher twin of every pair left out of the
    candidates (its values duplicate the lower twin's): what has to clear MIN_MARGIN for the states to be defined."""
    lp, states, margins = viterbi(startprob, transmat, B)
    keep = np.array([k for k in range(B.shape[1]) if k not in higher_twins(twins)])
    lpi, lA = _log(startprob), _log(transmat)
    T = B.shape[0]
    lat = np.empty(B.shape)
    lat[0] = lpi + B[0]
    for t in range(1, T):
        lat[t] = (lat[t - 1][:, None] + lA).max(axis=0) + B[t]
    reduced = np.empty(T)
    reduced[T - 1] = _margin(lat[T - 1][keep])
    for t in range(T - 2, -1, -1):
        reduced[t] = _margin((lat[t] + lA[:, states[t + 1]])[keep])
    return lp, states, margins, reduced


def impossible_model():
    """Three states; an observation of 1e200 has log-density -inf under every state, so every path through it is -inf."""
    start = np.array([0.5, 0.5, 0.0])
    trans = np.array([[0.5, 0.5, 0.0], [0.25, 0.5, 0.25], [0.0, 0.5, 0.5]])
    means = np.array([[0.0, 0.0], [2.0, -1.0], [-2.0, 1.0]])
    covars = np.ones((3, 2))
    return start, trans, means, covars


def twin_sequence(model, twins, T, seed, dwell=12):
    """T windows along a seeded path that spends about half its time in the lower twins, so that tied decisions are
    frequent everywhere (a tie occurs wherever the decoded state is a lower twin)."""
    start, trans, means, covars = model
    rng = np.random.default_rng(seed)
    K, D = means.shape
    lower = [a for a, _ in twins]
    path = np.empty(T, dtype=np.int64)
    s = lower[0]
    for t in range(T):
        if t and rng.random() < 1.0 / dwell:
            s = int(rng.choice(lower)) if rng.random() < 0.5 else int(rng.integers(K))
        path[t] = s
    return means[path] + np.sqrt(covars[path]) * 0.7 * rng.standard_normal((T, D))


def logprob_ld(startprob, transmat, B_ld):
    """The best path's log-probability by the (max,+) recursion in np.longdouble over log-densities B_ld."""
    with np.errstate(divide="ignore"):
        lpi, lA = np.log(np.asarray(startprob, dtype=np.longdouble)), np.log(np.asarray(transmat, dtype=np.longdouble))
    lat = lpi + B_ld[0]
    for t in range(1, B_ld.shape[0]):
        lat = (lat[:, None] + lA).max(axis=0) + B_ld[t]
    return lat.max()


TWIN_T = (1, 2, 8, 9, 257, 513)
BLOCK_ROWS = (1, 2, 7, 8, 9, 255, 256, 257, 300, 512)
# (n_states, n_dims, twin pairs, seed): KP = 2, 4, 8, 16, 32, 32; the seeds are those for which every decision between
# states that are not twins clears MIN_MARGIN at every length of TWIN_T (asserted in tests/test_model_edges_ref_cpu.py)
TWIN_CASES = (
    (2, 3, ((0, 1),), 1),
    (3, 8, ((1, 2),), 1),
    (5, 9, ((0, 3), (1, 4)), 3),
    (9, 7, ((2, 7),), 11),
    (17, 12, ((0, 16),), 1),
    (32, 5, ((30, 31), (0, 15)), 3),
)


def twin_case(i, T):
    """(model, twins, X [T][D]) of TWIN_CASES[i] at length T."""
    K, D, twins, seed = TWIN_CASES[i]
    model = twin_model(K, D, seed, twins)
    return model, twins, twin_sequence(model, twins, T, seed + 7 * T)


def offset_rows(n, d, seed=5):
    """[d][n] features whose row 0 is 1e8 + 1e-6 x noise (a deviation of 1e-6 under an offset fourteen decades above it);
    the other rows are benign."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((d, n)) * 2.0 + 1.0
    F[0] = 1e8 + 1e-6 * rng.standard_normal(n)
    return np.ascontiguousarray(F)


# (case, T, block_rows): 65 and more segments per sequence
SEGMENT_CASES = ((1, 200, 1), (2, 131, 2), (2, 130, 2), (3, 66 * 7 + 3, 7), (5, 65 * 8, 8), (0, 1000, 9))


def segment_case(case, T):
    """(model, twins, X [T][D]): the T = 513 sequence of a twin case cut to T rows, or two of them joined."""
    model, twins, X = twin_case(case, 513)
    if T > 513:
        X = np.concatenate([X, X])
    return model, twins, X[:T]


def ragged_parts():
    """(model, twins, sequences): length-1 sequences between multi-segment ones of twin case 2."""
    model, twins, X513 = twin_case(2, 513)
    X257, X9 = twin_case(2, 257)[2], twin_case(2, 9)[2]
    return model, twins, [X513[:1], X513, X257[5:6], X9, X257, X9[:2], X513[100:101]]


def impossible_batch():
    """(model, X, lengths): sequences 1 and 3 hold an observation of 1e200 (see impossible_model)."""
    rng = np.random.default_rng(4)
    good = rng.standard_normal((20, 2)) * 1.5
    bad = good.copy()
    bad[11, 0] = 1e200
    return impossible_model(), np.concatenate([good, bad, good[:1], bad[11:12], good]), [20, 20, 1, 1, 20]
