"""The inputs of tests/test_onset_edges_gpu.py without a device (tests/onset_edge_cases.py): that each is what it claims, that the
case table as a whole reaches every kernel path it was written for -- the tie terms of onset_select_kernel and
onset_threshold_kernel at both ends, the last byte of block_select, the negative branch of order_key, the seams of compact_frames,
the four remainders of the scaler's unrolled loops, both clamps and both branches of stage 4 -- the margins the comparisons rely
on, and, for the exact kinds, that the restated limits equal NumPy's bit for bit.  A case that stops being what it claims fails
here; it is not excused."""
import numpy as np
import pytest

import onset_edge_cases as E
import onset_ref
import onset_svm_ref
from pyaudioanalysis_amd import audioSegmentation as aS

STAGE12 = E.stage12_cases()


# ---- stages 1 and 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STAGE12))
def test_exact_kinds_have_numpys_limits_bit_for_bit(name):
    st = STAGE12[name]
    ref = onset_ref.training_sets(st)
    assert (ref["quiet_limit"], ref["loud_limit"]) == E.numpy_limits(st[1]), name
    quiet, loud = aS._energy_extremes(st)
    assert np.array_equal(quiet, st[:, ref["quiet_idx"]]) and np.array_equal(loud, st[:, ref["loud_idx"]]), name
    feats = ref["features"]
    assert np.array_equal(feats, np.vstack([quiet.T, loud.T]))
    if len(feats) >= 3:
        scale = np.sqrt(feats.var(axis=0))
        scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
        assert np.array_equal(ref["mean"], feats.mean(axis=0)) and np.array_equal(ref["scale"], scale), name


def test_coarse_dyadic_sums_are_exact_and_reach_the_high_end_tie_terms():
    paths = {}
    for c in E.COARSE_BITS:
        for T in E.COARSE_FRAMES:
            e = STAGE12["coarse_c%d_T%d" % (c, T)][1]
            k = e * 2.0 ** c
            assert np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() < 2 ** c and len(e) == T
            paths[(c, T)] = E.rank_paths(e)
    every = list(paths.values())
    assert any(1 < p["c_max"] < p["tenth"] and not p["max_is_hi"] for p in every)        # (c_max - 1) v_max is neither 0 nor all
    assert any(p["hi_ties"] >= 2 and not p["max_is_hi"] for p in every)                  # (tenth - c_gt) v_hi is not v_hi
    assert any(p["max_is_hi"] and not p["all_equal"] for p in every)                     # the second branch, not by all_equal
    assert any(p["low_ties"] >= 2 for p in every)
    assert any(p["c_max"] == 2 and p["low_ties"] >= 2 and not p["max_is_hi"] for p in every)
    # the largest clip has sums beyond the rank values AND ties at them at both ends, over many frames per thread
    big = paths[(6, 4099)]
    assert 2 <= big["low_ties"] < big["tenth"] and 2 <= big["hi_ties"] < big["tenth"] and 1 < big["c_max"] < big["tenth"]


@pytest.mark.parametrize("T", E.CLUSTER_FRAMES)
def test_bit_clusters_differ_in_the_last_key_bytes_only(T):
    for kind in E.CLUSTER_KINDS:
        e = STAGE12["cluster_%s_T%d" % (kind, T)][1]
        ranked = np.sort(e)
        keys = E.key_bytes(ranked)
        assert len(np.unique(e)) == T and np.all(keys[:, :6] == keys[0, :6]), kind
        assert np.all(np.diff(ranked.view(np.uint64).astype(np.int64)) >= 1) and ranked[-1] - ranked[0] < 1e-10
        ql, ll = E.numpy_limits(e)
        # tenth = 2: (a + b) / 2 is one rounded addition and an exact halving, the loud mean is one value; + 1e-15 rounds away
        assert ql == (ranked[0] + ranked[1]) / 2 + 1e-15 == (ranked[0] + ranked[1]) / 2 and ll == ranked[-2] + 1e-15 == ranked[-2], kind
        ref = onset_ref.training_sets(STAGE12["cluster_%s_T%d" % (kind, T)])
        assert len(ref["quiet_idx"]) in (1, 2) and len(ref["loud_idx"]) == 2, kind
        if kind == "skip_one":
            assert np.all(keys[:, 6] == keys[0, 6]) and keys[0, 7] == 0
            assert ql not in e and ranked[0] < ql < ranked[1] and len(ref["quiet_idx"]) == 1      # an off-by-one rank moves a set
        if kind == "bucket_255":
            assert np.all(keys[:, 6] == keys[0, 6]) and keys[-1, 7] == 255 and keys[-2, 7] == 254
        if kind == "rank_255":
            # the maximum's bucket alone cannot show in a limit at tenth = 2 (a maximum mistaken for ranked[-2] takes the v_max ==
            # v_hi branch to the same value), so here the LOW rank value lies in bucket 255, above bucket 252 and below a carry
            assert keys[0, 7] == 252 and keys[1, 7] == 255 and keys[2, 7] == 0 and keys[2, 6] == keys[0, 6] + 1
            two_up = (ranked[:1].view(np.uint64) + np.uint64(2)).view(np.float64)[0]
            assert ql == two_up and ql not in e and len(ref["quiet_idx"]) == 1
        if kind == "carry":
            assert keys[0, 7] == 255 and keys[1, 7] == 0 and keys[1, 6] == keys[0, 6] + 1         # ranks 0 and 1 across the carry
            assert len(np.unique(keys[:, 6])) == 2


@pytest.mark.parametrize("T", E.SIGNED_FRAMES)
def test_signed_dyadic_has_negative_energies_and_both_zeros_on_a_rank(T):
    e = STAGE12["signed_T%d" % T][1]
    assert np.array_equal(e * 8, np.round(e * 8)) and e.min() >= -1 and e.max() < 1 and (e < 0).sum() >= 2 and (e > 0).sum() >= 2
    zeros = e[e == 0]
    assert np.signbit(zeros).sum() >= 2 and (~np.signbit(zeros)).sum() >= 2
    ranked, tenth = np.sort(e), T // 10
    p = E.rank_paths(e)
    if T < 256:                                       # zeros of both signs are tied across the low rank, values lie below it
        assert ranked[tenth - 1] == 0 == ranked[tenth] and 2 <= p["low_ties"] < tenth
    else:                                             # .. and across the high rank, with values above it
        assert ranked[T - tenth] == 0 == ranked[T - tenth - 1] and 2 <= p["hi_ties"] < tenth and not p["max_is_hi"]
    ql, ll = E.numpy_limits(e)
    assert ql < 0 < ll                                # a negative limit too


def test_training_sets_cover_the_scalers_remainders_and_the_seams_of_the_compaction():
    paths = {name: E.energy_paths(st) for name, st in STAGE12.items()}
    assert {p["n_rows"] % 4 for p in paths.values() if p["n_rows"] >= 3} == {0, 1, 2, 3}
    assert any(p["n_rows"] < 4 for p in paths.values()) and any(p["n_rows"] > 2000 for p in paths.values())
    seam = paths["seam_T%d" % E.SEAM_FRAMES]
    assert seam["empty_chunk"] and seam["seam_255"] and seam["seam_0"]
    ref = onset_ref.training_sets(STAGE12["seam_T%d" % E.SEAM_FRAMES])
    assert {255, 256, 1023, 1024} <= set(ref["quiet_idx"].tolist()) and not np.any((ref["quiet_idx"] >= 512) & (ref["quiet_idx"] < 768))
    assert {511, 512, 1029} <= set(ref["loud_idx"].tolist()) and ref["loud_idx"].min() >= 256


# ---- stages 4 and 5 ---------------------------------------------------------------------------------------------------------------
def test_single_clip_cases_keep_their_margins():
    cases = E.stage45_cases()
    assert len(cases) == len(E.PIECEWISE_CASES) + len(E.SATURATED_WIDTHS) + 1
    for name, (st, model, width, weight, ref, paths) in cases.items():
        T = st.shape[1]
        assert ref["exit_margin"] > onset_svm_ref.MARGIN_MIN and ref["thr_margin"] > 1e-6 and 0 < len(ref["active"]) < T, name
        again = onset_ref.activity(st, model, width, weight)
        assert np.array_equal(again["prob"], ref["prob"]) and again["threshold"] == ref["threshold"], name


def test_piecewise_constant_frames_tie_across_both_ranks():
    cases = E.stage45_cases()
    low, high = [], []
    for T, width, weight in E.PIECEWISE_CASES:
        st, model, w, wt, ref, paths = cases["piecewise_T%d_w%d" % (T, width)]
        assert st.shape == (onset_ref.N_DIMS, T) and (w, wt) == (width, weight) and np.all(st[1] >= 0)
        n_columns = len(np.unique(st.T, axis=0))
        # few distinct columns.  (The restatement's matrix product may round equal columns differently by their position -- seen:
        # 121 values from 120 columns at T = 4099 -- so the ties are counted on its smoothed row, below, not assumed.)
        assert n_columns < T // 8 and len(np.unique(ref["raw_prob"])) < T // 8
        ranked, tenth = np.sort(ref["prob"]), T // 10
        if ranked[tenth - 1] == ranked[tenth] and paths["low_ties"] >= 2:
            low.append(width)
        if ranked[T - tenth] == ranked[T - tenth - 1] and paths["hi_ties"] >= 2:
            high.append(width)
        # and not the whole tenth: values strictly beyond the rank value are summed beside the tie term
        assert paths["low_ties"] < tenth and paths["hi_ties"] < tenth
    assert len(low) >= 2 and max(low) >= 3 and len(high) >= 2 and max(high) >= 3
    assert len(low) == len(high) == len(E.PIECEWISE_CASES)                              # as found: every case ties at both ends


def test_the_saturated_model_hits_both_clamps_and_both_branches():
    cases = E.stage45_cases()
    for width in E.SATURATED_WIDTHS:
        st, model, _, _, ref, paths = cases["saturated_w%d" % width]
        n_low, n_high, n_pos, n_neg = E.saturation(st, model)
        tenth = st.shape[1] // 10
        assert st.shape[1] == 257 and n_low > tenth and n_high > tenth and n_pos > tenth and n_neg > tenth
        assert len(np.unique(ref["raw_prob"])) < tenth
        if width < 3:                                 # untouched: the whole lowest and the whole highest tenth sit on a clamp
            assert paths["low_ties"] == tenth and paths["hi_ties"] == tenth
        else:
            assert paths["low_ties"] >= 2 and paths["hi_ties"] >= 2
    assert cases["saturated_w2"][0] is not cases["saturated_w9"][0] and np.array_equal(cases["saturated_w2"][0], cases["saturated_w9"][0])


def test_the_wide_case_smooths_over_the_whole_of_a_long_clip():
    st, model, width, weight, ref, _ = E.stage45_cases()["wide_T%d" % E.WIDE_CASE[0]]
    assert st.shape[1] == width == 300 and width > 256          # more frames than threads, a box that reaches both reflections


def test_short_clips_keep_their_margins_and_cut_into_several_chunks():
    mats, models, widths, weights, refs = E.short_clips()
    assert len(mats) == len(models) == len(widths) == len(weights) == len(refs) == E.N_SHORT == 200
    frames = np.array([m.shape[1] for m in mats])
    assert frames.min() == 20 and frames.max() == 45 and frames[0] == 20 and frames[-1] == 20 and len(set(frames.tolist())) > 20
    kinds = {2: 0, 3: 0, "T": 0}
    for st, width, weight, ref in zip(mats, widths, weights, refs):
        T = st.shape[1]
        assert ref["exit_margin"] > onset_svm_ref.MARGIN_MIN and ref["thr_margin"] > 1e-6 and 0 < len(ref["active"]) < T
        assert width in (2, 3, T)
        kinds["T" if width == T else width] += 1
    assert min(kinds.values()) >= 40 and len(set(weights)) == 4
    # what the library counts for a clip is at least its matrix: the bound of the chunked run cuts the call into more than 15 chunks
    assert frames.sum() * onset_ref.N_DIMS * 8 > 15 * E.SHORT_CHUNK_BYTES
    assert frames.max() * (onset_ref.N_DIMS * 8 + 19) + 4096 < E.SHORT_CHUNK_BYTES // 4       # and several clips to a chunk
