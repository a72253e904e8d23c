"""The kernels of silence_removal_batch (pyaudioanalysis_amd/csrc/kernels_onset.hpp) at ties, bit clusters and saturation: the
inputs of tests/onset_edge_cases.py through onset_training_sets and onset_activity against NumPy's sort and the restatement
tests/onset_ref.py, and the whole call on the golden with digital silence against a loop of the host functions.  -m gpu.  That the
inputs reach the paths they were written for, and the margins these comparisons rely on, is asserted on the CPU in
tests/test_onset_edges_ref_cpu.py (the golden's margins in tests/test_onset_batch_cpu.py)."""
import numpy as np
import pytest

import onset_edge_cases as E
import onset_ref
from pyaudioanalysis_amd import audioSegmentation as aS, audioTrainTest as aT
from test_onset_batch_gpu import TIGHT, host_loop, load, same_record

pytestmark = pytest.mark.gpu

ACTIVITY_KEYS = ("raw_prob", "prob", "threshold", "active")
STAGE12_GROUPS = ("coarse_c1", "coarse_c3", "coarse_c6", "cluster_skip_one", "cluster_bucket_255", "cluster_carry", "cluster_rank_255", "signed",
                  "seam")


# ---- stages 1 and 2: every kind is exact, the limits are NumPy's bit for bit --------------------------------------------------
@pytest.mark.parametrize("group", STAGE12_GROUPS)
def test_exact_selection_and_training_sets_against_numpy(gpu_lib, group):
    cases = {name: st for name, st in E.stage12_cases().items() if name.startswith(group + "_")}
    assert cases
    got = aS.onset_training_sets(list(cases.values()))
    for (name, st), g in zip(cases.items(), got):
        ref = onset_ref.training_sets(st)
        for mine, theirs in zip((g["quiet_limit"], g["loud_limit"]), E.numpy_limits(st[1])):
            print(name, repr(mine), repr(theirs), mine - theirs)
            assert mine == theirs, name
        assert np.array_equal(g["quiet_idx"], ref["quiet_idx"]) and np.array_equal(g["loud_idx"], ref["loud_idx"]), name
        assert np.array_equal(g["quiet_flags"], st[1] <= ref["quiet_limit"]) and np.array_equal(g["loud_flags"], st[1] >= ref["loud_limit"]), name
        quiet, loud = aS._energy_extremes(st)
        feats = np.vstack([quiet.T, loud.T])
        assert np.array_equal(g["features"], feats), name
        assert np.array_equal(g["mean"], ref["mean"]) and np.array_equal(g["scale"], ref["scale"]), name
        if len(feats) >= 3:             # NumPy's own reductions, bit for bit
            scale = np.sqrt(feats.var(axis=0))
            scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
            assert np.array_equal(g["mean"], feats.mean(axis=0)) and np.array_equal(g["scale"], scale), name
    alone = aS.onset_training_sets([list(cases.values())[-1]])[0]
    assert same_record(alone, got[-1], ("quiet_limit", "loud_limit", "quiet_idx", "loud_idx", "features", "mean", "scale"))


# ---- stages 4 and 5 with exact ties ---------------------------------------------------------------------------------------------
def check_activity(name, g, ref, width):
    d_raw, d_prob = np.max(np.abs(g["raw_prob"] - ref["raw_prob"])), np.max(np.abs(g["prob"] - ref["prob"]))
    print(name, d_raw, d_prob, abs(g["threshold"] - ref["threshold"]))
    assert d_raw <= TIGHT and d_prob <= TIGHT, name
    assert abs(g["threshold"] - ref["threshold"]) <= 1e-12, name
    assert np.array_equal(g["active"], ref["active"]), name
    if width < 3:
        assert np.array_equal(g["prob"], g["raw_prob"]), name


def test_tied_and_saturated_probabilities_against_the_restatement(gpu_lib):
    cases = E.stage45_cases()
    mats, models = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
    widths, weights = [c[2] for c in cases.values()], [c[3] for c in cases.values()]
    got = aS.onset_activity(mats, models, widths, weights)
    for (name, (st, model, width, weight, ref, paths)), g in zip(cases.items(), got):
        check_activity(name, g, ref, width)
        mine = E.rank_paths(g["prob"])
        print(name, paths, mine)
        if not name.startswith("wide"):
            # identical columns go through one sequence of operations on the device too: its own row is tied across both ranks,
            # so the tie terms of the threshold carry what the comparison above sees
            assert mine["low_ties"] >= 2 and mine["hi_ties"] >= 2, name
        if name.startswith("piecewise"):
            assert len(np.unique(g["raw_prob"])) == len(np.unique(st.T, axis=0)), name      # one value per distinct column
        if name.startswith("saturated"):
            for end in (np.min, np.max):            # the frames on each clamp are exactly equal, and as many as the restatement's
                assert np.sum(g["raw_prob"] == end(g["raw_prob"])) == np.sum(ref["raw_prob"] == end(ref["raw_prob"])) > 100, name
    for k, name in enumerate(cases):
        one = aS.onset_activity([mats[k]], [models[k]], widths[k], weights[k])[0]
        assert same_record(one, got[k], ACTIVITY_KEYS), name
    cut = aS.onset_activity(mats, models, widths, weights, chunk_bytes=1 << 20)       # the two clips of 4099 frames alone
    assert all(same_record(a, b, ACTIVITY_KEYS) for a, b in zip(got, cut))


def test_two_hundred_short_clips_in_one_call(gpu_lib):
    mats, models, widths, weights, refs = E.short_clips()
    got = aS.onset_activity(mats, models, widths, weights)
    assert len(got) == E.N_SHORT
    for k, (g, ref) in enumerate(zip(got, refs)):       # every clip's first and last frame find their own model
        check_activity("clip %d" % k, g, ref, widths[k])
    for k in (0, E.N_SHORT // 2, E.N_SHORT - 1):
        one = aS.onset_activity([mats[k]], [models[k]], widths[k], weights[k])[0]
        assert same_record(one, got[k], ACTIVITY_KEYS), k
    cut = aS.onset_activity(mats, models, widths, weights, chunk_bytes=E.SHORT_CHUNK_BYTES)
    assert all(same_record(a, b, ACTIVITY_KEYS) for a, b in zip(got, cut))


# ---- the whole call on the golden with digital silence ----------------------------------------------------------------------------
def test_the_batch_equals_a_loop_of_the_host_functions_on_digital_silence(gpu_lib):
    """test_the_batch_equals_a_loop_of_the_host_functions of tests/test_onset_batch_gpu.py for silence_synth_gaps: zero-energy
    frames, identical training rows and tied probabilities"""
    g = load("silence_synth_gaps")
    clips = [g["signal"]]
    args = (int(g["fs"]), float(g["st_win"]), float(g["st_step"]), float(g["smooth_window"]), float(g["weight"]))
    np.random.seed(int(g["seed"]))
    want = host_loop(clips, *args)
    np.random.seed(int(g["seed"]))
    segs, details = aS.silence_removal_batch(clips, *args, return_details=True)
    for w, s, d in zip(want, segs, details):
        assert d["seed"] == w["seed"]
        assert np.array_equal(w["st"][:, d["quiet_idx"]], w["quiet"]) and np.array_equal(w["st"][:, d["loud_idx"]], w["loud"])
        assert np.array_equal(d["mean"], w["mean"]) and np.array_equal(d["scale"], w["scale"])
        assert np.array_equal(d["alpha_y"], w["alpha_y"]) and d["rho"] == w["rho"]
        assert d["prob_a"] == w["prob_a"] and d["prob_b"] == w["prob_b"]
        print(np.max(np.abs(d["raw_prob"] - w["raw"])), np.max(np.abs(d["prob"] - w["prob"])), E.rank_paths(w["st"][1]), E.rank_paths(d["prob"]))
        assert np.max(np.abs(d["raw_prob"] - w["raw"])) <= TIGHT and np.max(np.abs(d["prob"] - w["prob"])) <= TIGHT
        assert s == w["segments"]
        assert d["status"][0] == aT.SMO_CONVERGED and len(d["alpha_y"]) == len(d["quiet_idx"]) + len(d["loud_idx"])
    got = np.array(segs[0], dtype=np.float64).reshape(-1, 2)
    assert got.shape == g["segments"].shape and np.allclose(got, g["segments"], rtol=0, atol=1e-9)
