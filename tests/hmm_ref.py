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
