"""NumPy restatement of pyAudioAnalysis's k-nearest-neighbour classifier (audioTrainTest.Knn.classify) with a defined tie
order -- the CPU second opinion for the GPU kNN kernel (pyaudioanalysis_amd/csrc/kernels_knn.hpp).  Test helper, not part
of the package.

Per query x (already standardised): the squared Euclidean distance to every training row in the difference form, the rows
in ascending (squared distance, training index), the first k of them vote; P[c] is the number of votes for the integer
c in 0..n_classes-1 divided by k (n_classes = the number of distinct labels; a label that is no such integer votes for no
class; with fewer than k rows the division is still by k) and the label is the first maximum of P.  The reference sorts
the distances with np.argsort, whose order among equal distances is not defined; see ambiguous()."""
import numpy as np

AMBIGUOUS_RTOL = 1e-12


def label_indices(labels):
    """(class index of every training row or -1, n_classes) as Knn.classify counts them."""
    raw = np.asarray(labels).reshape(-1)
    n_classes = int(np.unique(raw).shape[0])
    out = np.full(raw.shape[0], -1, dtype=np.int64)
    if raw.dtype.kind in "biuf":
        v = raw.astype(np.float64)
        ok = (v == np.floor(v)) & (v >= 0) & (v < n_classes)
        out[ok] = v[ok].astype(np.int64)
    return out, n_classes


def squared_distances(features, X):
    """[n_vec][n_train] sum_d (t_d - x_d)^2 of X [n_vec][n_dims] to features [n_train][n_dims]."""
    T = np.asarray(features, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    return np.stack([np.sum((T - x) ** 2, axis=1) for x in X])


def classify(features, labels, k, X):
    """(labels [n_vec] int64, P [n_vec][n_classes], neighbours [n_vec][k] with -1 past n_train) of the rows of X."""
    lab, n_classes = label_indices(labels)
    D = squared_distances(features, X)
    n_vec, n_train = D.shape
    idx = np.empty(n_vec, dtype=np.int64)
    P = np.zeros((n_vec, n_classes))
    nb = np.full((n_vec, k), -1, dtype=np.int64)
    rows = np.arange(n_train)
    for v in range(n_vec):
        order = np.lexsort((rows, D[v]))[:k]
        nb[v, :order.shape[0]] = order
        votes = lab[order]
        for c in range(n_classes):
            P[v, c] = np.count_nonzero(votes == c) / float(k)
        idx[v] = int(np.argmax(P[v]))
    return idx, P, nb


def ambiguous(dist, labels, k):
    """Is a query's vote set undefined under the reference's unstable sort?  dist: its distances to every training row
    (the reference's cdist values).  True when rows that tie with the k-th nearest (within AMBIGUOUS_RTOL relative) sit
    on both sides of the k boundary and do not all carry the same label."""
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    if dist.shape[0] <= k:
        return False
    lab = np.asarray(labels).reshape(-1)
    order = np.argsort(dist, kind="stable")
    kth = dist[order[k - 1]]
    near = np.abs(dist - kth) <= AMBIGUOUS_RTOL * abs(kth)
    pos = np.empty_like(order)
    pos[order] = np.arange(order.shape[0])
    inside, outside = near & (pos < k), near & (pos >= k)
    return bool(inside.any() and outside.any() and np.unique(lab[near]).shape[0] > 1)
