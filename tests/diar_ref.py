"""NumPy / SciPy restatement of the clustering part of pyAudioAnalysis's speaker_diarization (audioSegmentation.py:815-1056,
lda_dim = 0) -- the CPU second opinion for pyaudioanalysis_amd/csrc/kernels_diar.hpp.  Test helper, not part of the package.

Steps (X = the D x N matrix of mid-term features and SVM probabilities, one column per window):

  3  Z = StandardScaler().fit_transform(X.T)                         N x D, population std, a constant row gets scale 1
  4  s = column sums of squareform(pdist(Z.T)) -- distances between the D feature ROWS; keep the DIMENSIONS with
     s < 1.1 mean(s) (windows are never removed)                                                        -> Zk, N x D'
  5  KMeans(n_clusters = k, one initialisation) for k = 2..9 (or [n_speakers]): Lloyd, nearest centre by
     sum_d (z_d - c_d)^2 with the lowest index among equal minima, max_iter 300, tol = 1e-4 mean(var(Zk, axis = 0)) on the
     summed squared centre shift, stop at once when no label changes, empty clusters moved to the windows farthest from
     their centres (farthest first, lowest index among equals); when the run stops for another reason than unchanged labels
     the windows are assigned once more to the final centres; inertia from the final centres and labels.
  6  share s_c = n_c / N; s_c < 0.02: a_c = b_c = 0; else a_c = mean(pdist(Zk[cls == c].T)) s_c (feature rows again) and
     b_c = min over c2 != c of mean(cdist(Zk[cls == c], Zk[cls == c2])) (s_c + s_c2) / 2;
     sil_c = (b_c - a_c) / (max(b_c, a_c) + 1e-5); score(k) = mean_c sil_c; imax = first arg max.
  7  HMM from train_hmm_compute_statistics(Z.T, labels of the LAST k tried) -- not of imax -- and Viterbi over the unfiltered Z
     (hmm_ref).
  8  scipy.signal.medfilt(states, 5) as float64.

Seeding (when no initial centres are given) is greedy k-means++ with 2 + int(ln k) candidates per step; its draws are
defined HERE (seed_indices), not by scikit-learn's version-specific order.

MARGINS say how far every decision is from flipping: step 4 min |s - 1.1 mean| / mean; every k-means iteration the smallest
relative gap (d2_second - d2_best) / d2_second between a window's two nearest centres; for b_c the relative gap between the two
smallest candidates; for imax the gap between the two best scores."""
import numpy as np

try:
    from scipy.spatial import distance
except ImportError:          # the np.longdouble restatements and the generators below need NumPy alone
    distance = None

import hmm_ref

K_RANGE = tuple(range(2, 10))


def standardize(X):
    """(Z [N][D], mean, var, scale) of X [D][N] as StandardScaler computes them."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    mean = X.sum(axis=1) / n
    dev = X - mean[:, None]
    var = ((dev ** 2).sum(axis=1) - dev.sum(axis=1) ** 2 / n) / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.where(constant, 1.0, np.sqrt(var))
    return (dev / scale[:, None]).T.copy(), mean, var, scale


def _rel_gap(second, best):
    if not np.isfinite(second):
        return np.inf
    return 0.0 if second == best else (second - best) / max(abs(second), abs(best))


def kept_dimensions(Z):
    """(indices of the kept dimensions, column sums, margin)."""
    D = Z.shape[1]
    s = distance.squareform(distance.pdist(Z.T)).sum(axis=0) if D > 1 else np.zeros(D)
    m = s.mean()
    kept = np.nonzero(s < 1.1 * m)[0]
    margin = float(np.min(np.abs(s - 1.1 * m)) / m) if m > 0 else 0.0
    return kept, s, margin


def sq_distances(Zk, C):
    """[N][K] squared distances in the difference form."""
    return ((Zk[:, None, :] - C[None, :, :]) ** 2).sum(axis=2) if Zk.shape[0] * C.shape[0] * Zk.shape[1] < 4e7 else \
        np.stack([((Zk - c) ** 2).sum(axis=1) for c in C], axis=1)


def _assign(Zk, C):
    d2 = sq_distances(Zk, C)
    labels = np.argmin(d2, axis=1)
    if C.shape[0] > 1:
        two = np.partition(d2, 1, axis=1)[:, :2]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(two[:, 1] == two[:, 0], 0.0, (two[:, 1] - two[:, 0]) / two[:, 1])
        margin = float(gap.min())
    else:
        margin = np.inf
    return labels, d2[np.arange(Zk.shape[0]), labels], margin


def kmeans(Zk, k, init, max_iter=300, tol=1e-4, dtype=np.float64):
    """Lloyd from the initial centres `init` [k][D'].  Returns a dict: labels, centers, n_iter, inertia, margin, strict.
    dtype np.longdouble: the same steps in extended precision (inertia is then a longdouble scalar)."""
    Zk = np.asarray(Zk, dtype=dtype)
    C = np.array(init, dtype=dtype).reshape(k, Zk.shape[1])
    n = Zk.shape[0]
    tol_abs = tol * np.mean(np.var(Zk, axis=0))
    old = np.full(n, -1)
    margin = np.inf
    strict = False
    n_iter = 0
    labels = old
    for it in range(max_iter):
        labels, d2, m = _assign(Zk, C)
        margin = min(margin, m)
        sums = np.zeros_like(C)
        np.add.at(sums, labels, Zk)
        cnt = np.bincount(labels, minlength=k).astype(np.int64)
        d2 = d2.copy()
        for e in np.nonzero(cnt == 0)[0]:
            far = int(np.argmax(d2))
            d2[far] = -1.0
            sums[labels[far]] -= Zk[far]
            sums[e] = Zk[far]
            cnt[e] = 1
            cnt[labels[far]] -= 1
        new = np.where(cnt[:, None] > 0, sums / np.maximum(cnt, 1)[:, None], C)
        shift = ((new - C) ** 2).sum()
        C = new
        n_iter = it + 1
        if np.array_equal(labels, old):
            strict = True
            break
        if shift <= tol_abs:
            break
        old = labels
    if not strict:
        labels, _, m = _assign(Zk, C)
        margin = min(margin, m)
    inertia = ((Zk - C[labels]) ** 2).sum()
    inertia = float(inertia) if dtype == np.float64 else inertia
    return {"labels": labels.astype(np.int64), "centers": C, "n_iter": n_iter, "inertia": inertia, "margin": margin,
            "strict": strict}


def seed_indices(Zk, k, random_state):
    """Greedy k-means++: the window indices of the k initial centres.  Draws: the first centre rs.randint(N); then per step
    rs.uniform(size = 2 + int(ln k)) * potential, looked up in the cumulative sum of the closest squared distances (clipped to
    N - 1); the candidate with the smallest new potential wins (first among equals)."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    n = Zk.shape[0]
    trials = 2 + int(np.log(k))
    idx = [int(rs.randint(n))]
    closest = ((Zk - Zk[idx[0]]) ** 2).sum(axis=1)
    for _ in range(1, k):
        pot = closest.sum()
        vals = rs.uniform(size=trials) * pot
        cand = np.minimum(np.searchsorted(np.cumsum(closest), vals), n - 1)
        d2 = np.stack([((Zk - Zk[c]) ** 2).sum(axis=1) for c in cand])
        new = np.minimum(closest[None, :], d2)
        best = int(np.argmin(new.sum(axis=1)))
        idx.append(int(cand[best]))
        closest = new[best]
    return np.array(idx, dtype=np.int64)


def pair_sums(Zk, labels, k):
    """S [k][k]: the sum of |z_i - z_j| over i in c, j in c2."""
    S = np.zeros((k, k))
    groups = [Zk[labels == c] for c in range(k)]
    for c in range(k):
        for c2 in range(k):
            if groups[c].shape[0] and groups[c2].shape[0]:
                S[c, c2] = distance.cdist(groups[c], groups[c2]).sum()
    return S


def silhouette(Zk, labels, k):
    """dict: a [k], b [k], sil [k], score, b_margin (the smallest relative gap between the two smallest b candidates)."""
    n = Zk.shape[0]
    share = np.array([np.count_nonzero(labels == c) for c in range(k)]) / float(n)
    a, b, b_margin = np.zeros(k), np.zeros(k), np.inf
    for c in range(k):
        if share[c] < 0.02:
            continue
        mine = Zk[labels == c]
        with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
            sup.filter(RuntimeWarning)
            a[c] = np.mean(distance.pdist(mine.T)) * share[c]
        cand = []
        for c2 in range(k):
            if c2 != c:
                with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
                    sup.filter(RuntimeWarning)
                    cand.append(np.mean(distance.cdist(mine, Zk[labels == c2])) * (share[c] + share[c2]) / 2.0)
        b[c] = min(cand)
        if len(cand) > 1:
            lo = np.sort(np.array(cand))[:2]
            b_margin = min(b_margin, _rel_gap(lo[1], lo[0]))
    sil = np.array([(b[c] - a[c]) / (max(b[c], a[c]) + 1e-5) for c in range(k)])
    return {"a": a, "b": b, "sil": sil, "score": float(np.mean(sil)), "b_margin": b_margin}


def medfilt5(x):
    """scipy.signal.medfilt(x, 5): zero-padded edges."""
    x = np.asarray(x, dtype=np.float64)
    p = np.concatenate((np.zeros(2), x, np.zeros(2)))
    return np.median(np.stack([p[i:i + x.shape[0]] for i in range(5)]), axis=0)


def evaluate(labels, labels_gt):
    """(cluster purity, speaker purity) of two label sequences, cut to the shorter one."""
    n = min(len(labels), len(labels_gt))
    u, li = np.unique(np.asarray(labels)[:n], return_inverse=True)
    g, gi = np.unique(np.asarray(labels_gt)[:n], return_inverse=True)
    table = np.zeros((len(u), len(g)))
    np.add.at(table, (li, gi), 1.0)
    return float(table.max(axis=1).sum() / n), float(table.max(axis=0).sum() / n)


def cluster(X, n_speakers, init_centers=None, random_state=None):
    """Steps 3-6.  init_centers: {k: [k][D']}; other k are seeded from `random_state`."""
    Z, mean, var, scale = standardize(X)
    kept, colsum, kept_margin = kept_dimensions(Z)
    Zk = np.ascontiguousarray(Z[:, kept])
    ks = list(K_RANGE) if n_speakers <= 0 else [int(n_speakers)]
    rs = np.random.RandomState(random_state)
    out = {"Z": Z, "mean": mean, "var": var, "scale": scale, "kept_dims": kept, "colsum": colsum, "kept_margin": kept_margin,
           "ks": ks, "per_k": {}}
    scores = []
    for k in ks:
        if init_centers is not None and k in init_centers:
            init = np.asarray(init_centers[k], dtype=np.float64)
        else:
            init = Zk[seed_indices(Zk, k, rs)]
        r = kmeans(Zk, k, init)
        r.update(silhouette(Zk, r["labels"], k))
        out["per_k"][k] = r
        scores.append(r["score"])
    out["scores"] = np.array(scores)
    out["imax"] = int(np.argmax(scores))
    top = np.sort(np.array(scores))[-2:]
    out["imax_margin"] = float(top[1] - top[0]) if len(scores) > 1 else np.inf
    return out


def smooth(Z, labels):
    """Steps 7-8: (HMM states, their margins, the median-filtered labels) from the labels of the last k."""
    priors, trans, means, cov = hmm_ref.train_statistics(Z.T, labels)
    _, states, margins = hmm_ref.decode(priors, trans, means, cov, Z)
    return states, margins, medfilt5(states)


def diarize(X, n_speakers, init_centers=None, random_state=None):
    """Steps 3-8: the details of cluster() plus hmm_states, hmm_margin, cls."""
    out = cluster(X, n_speakers, init_centers, random_state)
    last = out["per_k"][out["ks"][-1]]["labels"]
    states, margins, cls = smooth(out["Z"], last)
    out.update({"hmm_states": states, "hmm_margin": float(margins.min()), "cls": cls})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# restatements in a chosen precision (np.longdouble: the reference of the tolerance tests; NumPy alone) and the designed
# inputs of the edge suite (tests/test_diar_edges_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def standardize_p(X, dtype=np.longdouble):
    """(mean, var, scale, constant, bound) of X [D][N]: standardize()'s steps in `dtype`."""
    X = np.asarray(X, dtype=dtype)
    n = X.shape[1]
    mean = X.sum(axis=1) / n
    dev = X - mean[:, None]
    var = ((dev ** 2).sum(axis=1) - dev.sum(axis=1) ** 2 / n) / n
    eps = dtype(np.finfo(np.float64).eps)
    bound = n * eps * var + (n * mean * eps) ** 2
    constant = var <= bound
    return mean, var, np.where(constant, dtype(1), np.sqrt(var)), constant, bound


def pair_sums_p(Zk, labels, k, dtype=np.longdouble):
    """S [k][k] in `dtype`: the sum of |z_i - z_j| over i in c, j in c2 (difference form)."""
    Z = np.asarray(Zk, dtype=dtype)
    S = np.zeros((k, k), dtype=dtype)
    for i in range(Z.shape[0]):
        d = np.sqrt(((Z - Z[i]) ** 2).sum(axis=1))
        np.add.at(S[labels[i]], labels, d)
    return S


def dim_distances_p(Z, select=None, dtype=np.longdouble):
    """(column sums [D], mean over the D (D - 1) / 2 pairs) of the Euclidean distances between the FEATURE ROWS of
    Z [N][D] over the windows `select` (a boolean mask; None: all)."""
    Z = np.asarray(Z, dtype=dtype)
    if select is not None:
        Z = Z[select]
    D = Z.shape[1]
    M = np.sqrt(((Z.T[:, None, :] - Z.T[None, :, :]) ** 2).sum(axis=2)) if Z.shape[0] else np.zeros((D, D), dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return M.sum(axis=0), np.triu(M, 1).sum() / (dtype(0.5) * D * (D - 1))


PAIR_KS = (2, 3, 5, 8, 9, 16, 31, 32)


def hand_labels(n, ks=PAIR_KS):
    """labels [len(ks)][n] for one pair-sum launch over several k: a running pattern, then per k > 2 the last cluster EMPTY,
    cluster 1 a SINGLE window (n - 1, in the last tile) and -- for k >= 5 -- cluster 2 the eleven windows 3..13 alone (wholly
    inside the first 128-window tile)."""
    out = np.empty((len(ks), n), dtype=np.int32)
    t = np.arange(n)
    for i, k in enumerate(ks):
        lab = (t * 7 + i + t // 5) % k
        if k > 2:
            lab[lab == k - 1] = 0
        lab[lab == 1] = 0
        lab[n - 1] = 1
        if k >= 5:
            lab[lab == 2] = 3
            lab[3:14] = 2
        out[i] = lab
    return out


def scaler_rows(n, seed=9):
    """(X [7][n], expected constant flags): benign; offset 1e8 with unit noise; offset 1e6 with 1e-3 noise; nearly constant
    1 + 1e-9 noise (NOT constant by scikit-learn's bound); 1e6 + 1e-9 noise (constant by the bound: its variance is below
    (n mean eps)^2); exactly constant 2.5; exactly constant 0."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((7, n))
    X = np.stack([g[0] * 2.0 - 1.0, 1e8 + g[1], 1e6 + 1e-3 * g[2], 1.0 + 1e-9 * g[3], 1e6 + 1e-9 * g[4], np.full(n, 2.5),
                  np.zeros(n)])
    return np.ascontiguousarray(X), np.array([False, False, False, False, True, True, True])


def equidistant_case(lead=0):
    """(Zk [N][3], init [2 + lead][3]): 192 windows at (-2, 0), 256 at (2, 0) and 64 at (0, 4), which are exactly
    equidistant (d^2 = 20) from the centres (-2, 0) and (2, 0): they belong to the lower index.  Everything is a small
    dyadic number and the cluster sizes are powers of two, so every distance, sum, centre and the inertia is exact in FP64
    (FP64 and longdouble restatements agree bit for bit, asserted on the CPU).  lead: that many extra centres at
    (-50 - 10 i, 0), each with 256 windows on it, in front: the tie is then between clusters lead and lead + 1.
    The windows are shuffled; N = 512 + 256 lead spans several assign workgroups."""
    pts = [(-2.0, 0.0)] * 192 + [(2.0, 0.0)] * 256 + [(0.0, 4.0)] * 64
    init = [(-2.0, 0.0), (2.0, 0.0)]
    for i in range(lead):
        pts += [(-50.0 - 10 * i, 0.0)] * 256
        init.insert(i, (-50.0 - 10 * i, 0.0))
    Z = np.zeros((len(pts), 3))
    Z[:, :2] = np.array(pts)
    Z = Z[np.random.default_rng(3).permutation(len(pts))]
    C = np.zeros((len(init), 3))
    C[:, :2] = np.array(init)
    return np.ascontiguousarray(Z), C


FAR_TIES = {5: (0.0, 6.0), 6: (0.0, -6.0), 133: (-6.0, 0.0), 262: (0.0, 6.0)}


def two_empty_case():
    """(Zk [320][2], init [4][2]): centres 2 and 3 attract no window, so both are relocated in iteration 1, to the farthest
    windows.  Four windows tie for the farthest (d^2 = 36 from centre 0) at indices 5, 6, 133 and 262 -- three different
    points, so the order of the relocations shows in the centres: cluster 2 must take window 5 and cluster 3 window 6.
    Cluster 0 keeps 128 windows after giving two away, so its centre is dyadic; run with max_iter = 1."""
    Z = np.zeros((320, 2))
    Z[:, 0] = 8.0                                                 # cluster 1: all on its centre
    ordinary = [i for i in range(0, 320, 2) if i not in FAR_TIES][:126]     # cluster 0: 126 ordinary windows + the four
    Z[ordinary] = 0.0
    Z[ordinary[:26], 0] = 1.0
    for i, p in FAR_TIES.items():
        Z[i] = p
    init = np.array([[0.0, 0.0], [8.0, 0.0], [1000.0, 1000.0], [-1000.0, 1000.0]])
    return Z, init


def near_duplicate_case(n=200, d=9, seed=8):
    """(X [d][n], labels [n]): cluster 2 is 40 windows within 1e-9 of one another (in the last tile, across the tile edge
    when n > 128), clusters 0 and 1 ordinary windows."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((d, n)) * 1.5
    labels = (np.arange(n) % 2).astype(np.int32)
    dup = np.arange(110, 150)
    X[:, dup] = X[:, 110:111] + 1e-9 * rng.standard_normal((d, 40))
    labels[dup] = 2
    return np.ascontiguousarray(X), labels


def stage_case(seed=31):
    """(X [17][257], initial centres [3][kept dims]) for the stage dictionary of diarize_clusters_device: three planted
    speakers, the centres three windows of the standardised, filtered matrix."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((3, 17)) * 4.0
    path = rng.integers(3, size=257)
    X = np.ascontiguousarray((means[path] + rng.standard_normal((257, 17))).T * rng.uniform(0.5, 20.0, 17)[:, None])
    Z = standardize(X)[0]
    colsum, _ = dim_distances_p(Z, dtype=np.float64)
    kept = np.nonzero(colsum < 1.1 * colsum.mean())[0]
    first = [int(np.flatnonzero(path == c)[0]) for c in range(3)]
    return X, np.ascontiguousarray(Z[first][:, kept])
