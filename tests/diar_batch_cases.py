"""Inputs shared by tests/test_diar_batch_gpu.py and tests/test_diar_batch_cpu.py: the ragged clips of a diarization batch, the
clips whose data make the loop of single calls raise, and the comparison of one clip's batch result with its single call."""
import numpy as np

import diar_ref

# window counts: the largest k of the sweep, one more, the pair tile of 128, the 256-thread blocks and the HMM's 256-window
# blocks with their neighbours, and several blocks; BIG: past one and two of NumPy's 8192-element reduction chunks
RAGGED_N = (9, 10, 127, 128, 129, 255, 256, 257, 1025)
BIG_N = (8193, 16385)
DIMS = (9, 33, 148)                       # 33: one past the 32 dims the assign kernel stages at a time
FIXED_KS = (2, 8, 9, 16, 17, 32)          # the assign kernel's 8 / 16 / 32 instances on both sides of their edges
PER_K = ("labels", "centers", "n_iter", "inertia", "sil_a", "sil_b", "sil", "pair_sums")


def planted(seed, n, d, k, spread=4.0):
    """(M [d][n]): n windows around k planted speakers, as tests/test_diar_gpu.py plants them."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((k, d)) * spread
    path = rng.integers(k, size=n)
    return (means[path] + rng.standard_normal((n, d))).T.copy()


def ragged_clips(d, seed=0):
    """one planted clip per window count of RAGGED_N, all of d dims"""
    return [planted(1000 * d + 10 * i + seed, n, d, 2 + i % 4) for i, n in enumerate(RAGGED_N)]


def no_kept_dimension_clip(d, n=40, seed=3):
    """Every feature row is the same sequence: all dimension distances are exactly 0, so no column sum is below 1.1 times their
    mean (0 < 0) and the loop raises ValueError."""
    row = np.random.default_rng(seed).standard_normal(n)
    return np.tile(row, (d, 1))


def empty_cluster_clip(d=9, n=40, seed=5):
    """(M [d][n], init_centers {3: [3][kept]}): k-means with k = 3 ends with cluster 1 empty, so the labels are {0, 2} and the
    HMM statistics raise IndexError.  Windows 0 and 1 are one point P far from the rest.  Centre 0 starts off P but nearest to
    it, centre 1 far from everything, centre 2 on the rest.  Iteration 1 leaves cluster 1 empty; it takes the window farthest
    from its centre, which is window 0 (the lower of the two P windows, both farther from centre 0 than any other window is
    from centre 2); cluster 0 keeps one window, so centres 0 and 1 are both exactly P (2 P - P and P / 1 are exact).  In
    iteration 2 the two P windows tie at distance 0 and go to the lower index: no label changes and the run ends."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((d, n))
    M[:, :2] = 25.0 + np.arange(d)[:, None]
    Z, _, _, _ = diar_ref.standardize(M)
    kept, _, margin = diar_ref.kept_dimensions(Z)
    assert margin > 1e-6 and len(kept) >= 1
    Zk = Z[:, kept]
    init = np.stack([Zk[0] + 3.0, np.full(len(kept), 1e3), Zk[2:].mean(axis=0)])
    d2 = ((Zk[:, None, :] - init[None, :, :]) ** 2).sum(axis=2)
    assert np.all(np.argmin(d2, axis=1)[:2] == 0) and np.all(np.argmin(d2, axis=1)[2:] == 2)
    assert d2[0, 0] > d2[2:, 2].max()
    return M, {3: init}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_clusters(g, w, what):
    """the clustering half of the details of a clip of a batch against its single call, bit for bit"""
    assert same_bits(g["kept_dims"], w["kept_dims"]), (what, "kept_dims")
    assert g["ks"] == w["ks"] and g["imax"] == w["imax"], (what, "ks / imax")
    assert same_bits(g["scores"], w["scores"]), (what, "scores")
    for key in ("dim_colsum", "mean", "var", "scale"):
        assert same_bits(g[key], w[key]), (what, key)
    for k in w["ks"]:
        for key in PER_K:
            a, b = g[key][k], w[key][k]
            if key in ("n_iter", "inertia"):
                assert type(a) is type(b) and a == b, (what, key, k, a, b)
            else:
                assert same_bits(a, b), (what, key, k)


def assert_same_result(got, want, what):
    """(cls, details) of a clip of a batch against its single call: every entry the contract names, bit for bit"""
    (g_cls, g), (w_cls, w) = got, want
    assert same_bits(g_cls, w_cls), (what, "filtered labels")
    assert same_bits(g["hmm_states"], w["hmm_states"]), (what, "hmm_states")
    assert_same_clusters(g, w, what)


class TracedRandomState(np.random.RandomState):
    """records every draw the seeding makes: ("randint", n) and ("uniform", size) with their values"""

    def __init__(self, seed):
        super().__init__(seed)
        self.trace = []

    def randint(self, *args, **kw):
        v = super().randint(*args, **kw)
        self.trace.append(("randint", args[0], int(v)))
        return v

    def uniform(self, *args, **kw):
        v = super().uniform(*args, **kw)
        self.trace.append(("uniform", kw.get("size"), np.array(v)))
        return v
