"""The inputs of the edge tests of silence_removal_batch's kernels (pyaudioanalysis_amd/csrc/kernels_onset.hpp) and a classifier of
the kernel path each of them takes, shared by tests/test_onset_edges_ref_cpu.py (which establishes, without a device, that every
input is what it claims and that the table as a whole reaches every path) and tests/test_onset_edges_gpu.py (which runs them
through onset_training_sets and onset_activity).  Plain NumPy; the references are NumPy's sort and the restatement
tests/onset_ref.py, whose own tables stay as they are.  Imports nothing from the package.

(1) stages 1 and 2, energies whose sums are exact in any order, so that both limits are required bit for bit:
    coarse_dyadic   a few dyadic levels: long runs of ties at both ranks and at the maximum,
    bit_cluster     doubles one ulp apart next to 1024.0: the radix select has to tell them apart in its LAST byte, with a rank
                    value in bucket 255 and across a carry into the second-last byte,
    signed_dyadic   negative energies and both zeros: the other branch of order_key,
    seam            coarse dyadic energies placed so that flagged frames sit at both sides of compact_frames' 256-frame seams;
(2) stages 4 and 5 with exactly tied probabilities: piecewise-constant frames, a model that saturates at both clamps, a box as
    wide as a long clip, and 200 short clips in one call;
(3) nothing here: the whole call on the golden with digital silence needs no input of its own.
Test helper, not part of the package."""
import functools

import numpy as np

import onset_ref
import onset_svm_ref

N_DIMS = onset_ref.N_DIMS


# ---------------------------------------------------------------------------------------------------------------------------------
# the path classifier
# ---------------------------------------------------------------------------------------------------------------------------------
def rank_paths(row):
    """Which terms of the kernels' "sum strictly beyond the rank value + ties times that value" a row exercises.  With ranked =
    sort(row), v_lo = ranked[tenth - 1], v_hi = ranked[T - tenth], v_max = ranked[-1]:
    low_ties = tenth - #(x < v_lo), hi_ties = tenth - #(x > v_hi): the factors of v_lo and v_hi (1 where nothing is tied below /
    above the rank); c_max = #(x == v_max); max_is_hi = v_max == v_hi (onset_select_kernel's second branch); all_equal."""
    row = np.asarray(row, dtype=np.float64)
    T = len(row)
    tenth = T // 10
    ranked = np.sort(row)
    v_lo, v_hi, v_max = ranked[tenth - 1], ranked[T - tenth], ranked[-1]
    return dict(T=T, tenth=tenth, low_ties=int(tenth - np.sum(row < v_lo)), hi_ties=int(tenth - np.sum(row > v_hi)),
                c_max=int(np.sum(row == v_max)), max_is_hi=bool(v_max == v_hi), all_equal=bool(ranked[0] == ranked[-1]))


def energy_paths(st):
    """rank_paths of the energy row, the training-set size n_rows = n_quiet + n_loud, and what compact_frames meets: empty_chunk
    (a whole chunk of 256 frames without a flagged frame, before a chunk that has one: the running base is carried over it) and
    seam_255 / seam_0 (a flagged frame in the last / first lane of a chunk, a first lane past chunk 0)"""
    st = np.asarray(st, dtype=np.float64)
    ref = onset_ref.training_sets(st)
    out = rank_paths(st[1])
    out["n_rows"] = len(ref["quiet_idx"]) + len(ref["loud_idx"])
    out["empty_chunk"] = out["seam_255"] = out["seam_0"] = False
    for idx in (ref["quiet_idx"], ref["loud_idx"]):
        if len(idx) == 0:
            continue
        chunks = set((idx // 256).tolist())
        out["empty_chunk"] |= any(k not in chunks for k in range(int(idx.max()) // 256))
        out["seam_255"] |= bool(np.any(idx % 256 == 255))
        out["seam_0"] |= bool(np.any((idx % 256 == 0) & (idx > 0)))
    return out


def key_bytes(v):
    """the eight bytes, most significant first, of the order-preserving key the radix select sorts by (the sign bit set for a
    non-negative double, every bit flipped for a negative one); [len(v)][8] uint8"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    key = np.where(neg, ~b, b | np.uint64(1 << 63))
    return np.stack([((key >> np.uint64(s)) & np.uint64(255)).astype(np.uint8) for s in range(56, -8, -8)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) stages 1 and 2
# ---------------------------------------------------------------------------------------------------------------------------------
COARSE_BITS = (1, 3, 6)
COARSE_FRAMES = (20, 29, 30, 117, 400, 4099)
CLUSTER_KINDS = ("skip_one", "bucket_255", "carry", "rank_255")
CLUSTER_FRAMES = (20, 29)                  # tenth = 2: the low mean is (a + b) / 2, the loud mean the single value ranked[-2]
SIGNED_FRAMES = (117, 400)
SEAM_FRAMES = 1030                         # chunks of 256, 256, 256, 256 and 6 frames
BASE_1024 = np.float64(1024.0).view(np.uint64)         # 0x4090000000000000: one ulp is 2.3e-13, so + 1e-15 rounds away


def _matrix(rng, energy):
    st = rng.standard_normal((N_DIMS, len(energy)))
    st[1] = energy
    return np.ascontiguousarray(st)


def coarse_dyadic(c, T):
    """energies k 2^-c, k drawn from 0 .. 2^c - 1: every sum of them is exact"""
    rng = np.random.default_rng([9, c, T])
    e = rng.integers(0, 2 ** c, T) * 2.0 ** -c
    return _matrix(rng, e)


def cluster_offsets(kind, T, rng):
    """(last byte of the base pattern, the T offsets k added to it)"""
    if kind == "skip_one":                  # k = 0, 2, 3, 4, ..: (base + base + 2) / 2 = base + 1 is not present
        return 0x00, np.concatenate([[0], np.arange(2, T + 1)])
    if kind == "bucket_255":                # the largest pattern ends in 0xFF
        return 0xFF - (T - 1), np.arange(T)
    if kind == "rank_255":                  # 0xFC and 0xFF, then past the carry: rank tenth - 1 lies in bucket 255 above a filled bucket.
        return 0xFC, np.concatenate([[0, 3], np.arange(4, T + 2)])       # (m + m + 3) / 2 rounds to m + 2, an even pattern not present
    if kind == "carry":                    # 0xF8 + 7 = 0xFF, 0xF8 + 8 carries: the two smallest values lie on both sides
        return 0xF8, np.concatenate([[7, 8], 9 + rng.choice(55, T - 2, replace=False)])
    raise KeyError(kind)


def bit_cluster(kind, T):
    """energies whose bit patterns are (the pattern of 1024.0 with its last byte replaced) + k, shuffled"""
    rng = np.random.default_rng([10, CLUSTER_KINDS.index(kind), T])
    last, k = cluster_offsets(kind, T, rng)
    pattern = (BASE_1024 | np.uint64(last)) + np.asarray(k, dtype=np.uint64)
    return _matrix(rng, rng.permutation(pattern.view(np.float64)))


def signed_dyadic(T):
    """multiples of 1/8 in [-1, 1) with both zeros, laid out so that the zeros lie ON a rank: at T = 117 fewer negative values
    than a tenth, then zeros of both signs across rank tenth - 1; at T = 400 fewer positive values than a tenth, zeros of both
    signs across rank T - tenth"""
    rng = np.random.default_rng([11, T])
    tenth = T // 10
    few, zeros = tenth // 2, tenth
    n_neg, n_pos = (few, T - few - zeros) if T < 256 else (T - few - zeros, few)
    zero = np.where(np.arange(zeros) % 2 == 0, -0.0, 0.0)
    e = np.concatenate([-(rng.integers(1, 9, n_neg) / 8.0), zero, rng.integers(1, 8, n_pos) / 8.0])
    return _matrix(rng, rng.permutation(e))


def seam():
    """coarse dyadic energies (c = 6) of 1030 frames, placed by rank: the smallest at frames 255, 256, 1023, 1024, 0, 1, 2 ..,
    the largest at 1029, 511, 512, 1028, 1027 ..  So the quiet list has flagged frames in the last lane of chunk 0 and the first
    of chunk 1, none in chunk 2 and some in chunks 3 and 4, and the loud list has none in chunk 0"""
    T = SEAM_FRAMES
    rng = np.random.default_rng([12, T])
    ranked = np.sort(rng.integers(0, 64, T) * 2.0 ** -6)
    front, back = [255, 256, 1023, 1024], [512, 511, 1029]
    middle = [t for t in range(T) if t not in front and t not in back]
    e = np.zeros(T)
    e[np.array(front + middle + back)] = ranked
    return _matrix(rng, e)


@functools.lru_cache(maxsize=None)
def stage12_cases():
    """name -> short-term matrix [68][T] (shared: do not write to them)"""
    out = {}
    for c in COARSE_BITS:
        for T in COARSE_FRAMES:
            out["coarse_c%d_T%d" % (c, T)] = coarse_dyadic(c, T)
    for kind in CLUSTER_KINDS:
        for T in CLUSTER_FRAMES:
            out["cluster_%s_T%d" % (kind, T)] = bit_cluster(kind, T)
    for T in SIGNED_FRAMES:
        out["signed_T%d" % T] = signed_dyadic(T)
    out["seam_T%d" % SEAM_FRAMES] = seam()
    for st in out.values():
        st.setflags(write=False)
    return out


def numpy_limits(energy):
    """NumPy's own (quiet_limit, loud_limit): the means of the sorted row's ends + 1e-15"""
    ranked = np.sort(energy)
    tenth = len(ranked) // 10
    return ranked[:tenth].mean() + 1e-15, ranked[-tenth:-1].mean() + 1e-15


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) stages 4 and 5
# ---------------------------------------------------------------------------------------------------------------------------------
PIECEWISE_CASES = ((117, 2, 0.5), (400, 10, 0.3), (1030, 7, 0.5), (4099, 50, 0.5), (4099, 2, 0.99))
SATURATED_WIDTHS = (2, 9)
WIDE_CASE = (300, 300, 0.5)
N_SHORT, SHORT_FRAMES = 200, (20, 45)
SHORT_CHUNK_BYTES = 200000                 # the matrices alone are 544 bytes a frame: about 360 frames, ten clips, to a chunk


def margins_ok(ref, T):
    return ref["exit_margin"] > onset_svm_ref.MARGIN_MIN and ref["thr_margin"] > 1e-6 and 0 < len(ref["active"]) < T


def _level_probabilities(levels, model):
    mean, scale = np.asarray(model[4], dtype=np.float64), np.asarray(model[5], dtype=np.float64)
    return onset_svm_ref.predict(onset_ref.as_svm_model(model), levels, mean, scale)["prob1"]


def piecewise_case(T, width, weight):
    """(st, model, ref, paths): st[:, t] = level[:, segment(t)].  Identical columns give exactly equal raw probabilities, and inside
    a stretch longer than the box exactly equal smoothed ones (s += x * box is the same sequence of operations).  Two plateaus are
    longer than tenth + width and carry the SECOND lowest and the SECOND highest level, the lowest and the highest level get a short
    segment each: so the sorted smoothed row has values strictly below the low rank value AND a tie across the rank, and the same at
    the high end.  The first seed that keeps the margins of stage45_case and both ties."""
    tenth = T // 10
    long_len = tenth + width + max(3, tenth // 8)
    short_len = max(2, tenth // 3)
    for seed in range(50):
        rng = np.random.default_rng([46, T, int(width), int(round(weight * 100)), seed])
        n_other = max(3, (T - 2 * long_len - 2 * short_len) // max(2 * width, 25))
        cuts = np.sort(rng.choice(np.arange(1, T - 2 * long_len - 2 * short_len), n_other - 1, replace=False))
        lengths = np.diff(np.concatenate([[0], cuts, [T - 2 * long_len - 2 * short_len]])).tolist()
        roles = ["other"] * n_other
        for role in ("long_lo", "long_hi", "short_lo", "short_hi"):
            at = int(rng.integers(0, len(roles) + 1))
            roles.insert(at, role)
            lengths.insert(at, long_len if role.startswith("long") else short_len)
        levels = rng.standard_normal((N_DIMS, len(roles)))
        levels[1] = np.abs(levels[1])
        model = onset_ref.random_model(rng, np.repeat(levels, lengths, axis=1))
        order = np.argsort(_level_probabilities(levels, model))          # levels by their raw probability
        take = {"short_lo": order[0], "long_lo": order[1], "long_hi": order[-2], "short_hi": order[-1]}
        rest = iter(rng.permutation(order[2:-2]))
        pick = [take[r] if r in take else next(rest) for r in roles]
        st = np.ascontiguousarray(np.repeat(levels[:, pick], lengths, axis=1))
        assert st.shape == (N_DIMS, T)
        ref = onset_ref.activity(st, model, width, weight)
        paths = rank_paths(ref["prob"])
        if margins_ok(ref, T) and 2 <= paths["low_ties"] < tenth and 2 <= paths["hi_ties"] < tenth:
            st.setflags(write=False)
            return st, model, ref, paths
    raise AssertionError("no seed with clear margins and both ties for T = %d, width %d, weight %g" % (T, width, weight))


def saturated_case(width):
    """(st, model, ref, paths): 257 i.i.d. frames under a model with 12 times random_model's weights and A = -60: most frames land
    on the clamp 1e-7 or 1 - 1e-7 and both branches of the sigmoid are taken"""
    T = 257
    for seed in range(50):
        rng = np.random.default_rng([47, seed])
        st = rng.standard_normal((N_DIMS, T))
        st[1] = np.abs(st[1])
        st = np.ascontiguousarray(st)
        w, intercept, _, prob_b, mean, scale = onset_ref.random_model(rng, st)
        model = (w * 12.0, intercept, -60.0, prob_b, mean, scale)
        ref = onset_ref.activity(st, model, width, 0.5)
        if margins_ok(ref, T):
            st.setflags(write=False)
            return st, model, ref, rank_paths(ref["prob"])
    raise AssertionError("no seed with clear margins for the saturated model at width %d" % width)


def saturation(st, model):
    """(frames on the low clamp, frames on the high clamp, frames with fApB >= 0, frames with fApB < 0)"""
    r = onset_svm_ref.predict(onset_ref.as_svm_model(model), st, np.asarray(model[4]), np.asarray(model[5]))
    return (int(np.sum(r["r01"] == onset_svm_ref.CLIP)), int(np.sum(r["r01"] == 1 - onset_svm_ref.CLIP)), int(np.sum(r["fApB"] >= 0)),
            int(np.sum(r["fApB"] < 0)))


def wide_case():
    st, model, ref = onset_ref.stage45_case(*WIDE_CASE)
    return st, model, ref, rank_paths(ref["prob"])


@functools.lru_cache(maxsize=None)
def short_clips():
    """200 clips of 20 .. 45 frames, each with its own model, width (2, 3 or T) and weight: (mats, models, widths, weights, refs)"""
    rng = np.random.default_rng(48)
    frames = rng.integers(SHORT_FRAMES[0], SHORT_FRAMES[1] + 1, N_SHORT)
    frames[[0, N_SHORT // 2, N_SHORT - 1]] = (SHORT_FRAMES[0], SHORT_FRAMES[1], SHORT_FRAMES[0])
    kinds = rng.integers(0, 3, N_SHORT)
    weights = rng.choice([0.01, 0.3, 0.5, 0.99], N_SHORT)
    mats, models, widths, refs = [], [], [], []
    for k in range(N_SHORT):
        T = int(frames[k])
        width = (2, 3, T)[int(kinds[k])]
        st, model, ref = onset_ref.stage45_case(T, width, float(weights[k]), base_seed=1000 + 50 * k)
        st.setflags(write=False)
        mats.append(st), models.append(model), widths.append(width), refs.append(ref)
    return mats, models, widths, [float(w) for w in weights], refs


@functools.lru_cache(maxsize=None)
def stage45_cases():
    """name -> (st, model, width, weight, ref, paths) of the single-clip cases"""
    out = {}
    for T, width, weight in PIECEWISE_CASES:
        st, model, ref, paths = piecewise_case(T, width, weight)
        out["piecewise_T%d_w%d" % (T, width)] = (st, model, width, weight, ref, paths)
    for width in SATURATED_WIDTHS:
        st, model, ref, paths = saturated_case(width)
        out["saturated_w%d" % width] = (st, model, width, 0.5, ref, paths)
    st, model, ref, paths = wide_case()
    out["wide_T%d" % WIDE_CASE[0]] = (st, model, WIDE_CASE[1], WIDE_CASE[2], ref, paths)
    return out
