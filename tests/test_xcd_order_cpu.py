"""balanced_runs with an order of the XCD labels (csrc/lib_plan.hpp, csrc/lib_xcd_order.hpp), through the host debug entry: no
GPU.  A balanced plan of the 800-sample kernel has 256 workgroups of eight runs; waves w and w + 4 of a workgroup share a SIMD
and the workgroups of a label (workgroup mod 8) share an XCD.  With an order -- the eight labels, the slowest XCD's first -- the
SIMD pairs with the low iteration total are dealt label after label in that order, workgroup after workgroup; everything else
about the cut stays what the even spread gives.

"The multiset of run lengths equals the even spread's" cannot hold literally together with "the low-total pairs lie on a prefix of
the labels": a run's LENGTH depends on where it stands in its clip -- the first run has no halo frames inside, the last gives back
the quanta the clip does not have -- and those two runs stand in fixed workgroups.  In config 2 the even spread makes tile 0
short (68 frames: 17 iterations, no halo); an order that ranks label 0 among the fast ones must make it long (72 frames) and some
later run short instead (67 frames), so {68, 71} becomes {72, 67} with the same iteration counts.  The cuts are therefore compared
by the ITERATION counts of their runs, which is what "the same number of long and short runs" means; wherever the first and the
last run keep their counts the run lengths themselves are asserted to be the same multiset
(test_the_length_multiset_differs_only_through_the_first_and_last_run shows both cases occur).

What the even spread IS is pinned by tests/golden/balanced_runs_even_spread.json: the lengths the commit before the ordered cut
gave, recorded from that commit's library."""
import json
import os

import numpy as np

from pyaudioanalysis_amd import _ffi

WG_RUNS, NUM_CU, QUANTUM, MIN_RUN = 8, 256, 4, 16
IDENTITY = list(range(8))
ORDERS = [IDENTITY, IDENTITY[::-1], [3, 5, 1, 7, 0, 4, 2, 6], [6, 2, 7, 0, 5, 3, 1, 4], [1, 0, 3, 2, 5, 4, 7, 6]]


def cut(frames, cap, shrink, order=None, ordered_entry=True):
    arr = np.ascontiguousarray(frames, dtype=np.int64)
    out = np.zeros(8192, dtype=np.int32)
    lib = _ffi.lib()
    if ordered_entry:
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32).ctypes.data_as(_ffi.c_i32p)
        n = lib.paa_debug_balanced_runs_ordered(_ffi.as_i64p(arr), len(arr), cap, QUANTUM, shrink, WG_RUNS, NUM_CU, MIN_RUN, o,
                                                out.ctypes.data_as(_ffi.c_i32p), len(out))
    else:
        n = lib.paa_debug_balanced_runs(_ffi.as_i64p(arr), len(arr), cap, QUANTUM, shrink, WG_RUNS, NUM_CU, MIN_RUN,
                                        out.ctypes.data_as(_ffi.c_i32p), len(out))
    assert n >= 0
    return out[:n].copy()


def cap_of(frames, shrink):
    import ctypes
    arr = np.ascontiguousarray(frames, dtype=np.int64)
    cap, longest, runs = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    _ffi.check(_ffi.lib().paa_debug_run_plan_shrink(_ffi.as_i64p(arr), len(arr), QUANTUM, MIN_RUN, 256, shrink, WG_RUNS, NUM_CU,
                                                    ctypes.byref(cap), ctypes.byref(runs), ctypes.byref(longest)))
    return cap.value


def split(lens, frames):
    """The runs of every clip (they are consecutive in the list and sum to the clip's frames): [(first tile, lengths)]."""
    out, pos = [], 0
    for T in frames:
        acc, first = 0, pos
        while acc < T:
            acc += int(lens[pos])
            pos += 1
        assert acc == T, (acc, T)
        out.append((first, lens[first:pos]))
    assert pos == len(lens)
    return out


def iterations(l, shrink):
    return (l + np.where(np.arange(len(l)) > 0, shrink, 0) + QUANTUM - 1) // QUANTUM


def pairs_of(first, its):
    """SIMD pairs that lie inside a clip whose runs are tiles first .. first + len(its) - 1: [(workgroup, SIMD, total, tile of
    the first member)]."""
    out = []
    for j in range(first // WG_RUNS, (first + len(its) - 1) // WG_RUNS + 1):
        for s in range(4):
            a, b = j * WG_RUNS + s - first, j * WG_RUNS + s + 4 - first
            if a >= 0 and b < len(its):
                out.append((j, s, int(its[a] + its[b]), a))
    return out


# config 2's shape with one and with two halo frames; three clips; mostly long runs (config 2 has 1696 long of 2048) and mostly short
# ones (137 617 frames: 100 long of 2048)
SHAPES = [([143999], 1), ([143999], 2), ([40000, 60000, 43999], 1), ([137617], 1), ([139647], 1)]


def recorded_cuts():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "balanced_runs_even_spread.json")
    return json.load(open(path))["cuts"]


def test_no_order_is_the_even_spread():
    """Without an order both entries give, byte for byte, the lengths recorded from the commit before the ordered cut."""
    recorded = {(tuple(r["frames"]), r["shrink"]): r for r in recorded_cuts()}
    assert all((tuple(frames), shrink) in recorded for frames, shrink in SHAPES) and len(recorded) > len(SHAPES)
    for (frames, shrink), r in recorded.items():
        assert (r["quantum"], r["wg_runs"], r["num_cu"], r["min_run"]) == (QUANTUM, WG_RUNS, NUM_CU, MIN_RUN)
        cap = cap_of(list(frames), shrink)
        assert cap == r["run_cap"]
        want = np.array(r["lens"], dtype=np.int32)
        assert len(want) > 0 and int(want.sum()) == sum(frames)
        assert np.array_equal(cut(list(frames), cap, shrink, ordered_entry=False), want)
        assert np.array_equal(cut(list(frames), cap, shrink, None), want)
        # what is no permutation of the labels is no order either
        assert np.array_equal(cut(list(frames), cap, shrink, [0, 1, 2, 3, 4, 5, 6, 6]), want)
    l = cut([137617], cap_of([137617], 1), 1, None)
    assert int((iterations(l, 1) == iterations(l, 1).max()).sum()) < 200          # (the mostly short shape is one)


def test_ordered_cut_keeps_the_cut_and_moves_the_short_runs():
    for frames, shrink in SHAPES:
        cap = cap_of(frames, shrink)
        even = split(cut(frames, cap, shrink, None), frames)
        for order in ORDERS:
            lens = cut(frames, cap, shrink, order)
            assert lens.min() >= MIN_RUN and lens.max() <= cap
            rank = {label: r for r, label in enumerate(order)}
            for (first, l), (first_e, le) in zip(split(lens, frames), even):          # (split: per clip the runs sum to T)
                assert first == first_e and len(l) == len(le)
                its, its_e = iterations(l, shrink), iterations(le, shrink)
                assert np.array_equal(np.sort(its), np.sort(its_e)), (frames, order)
                if its[0] == its_e[0] and its[-1] == its_e[-1]:
                    assert np.array_equal(np.sort(l), np.sort(le)), (frames, order)
                assert its.max() - its.min() <= 1
                pairs = pairs_of(first, its)
                totals = np.array([p[2] for p in pairs])
                assert totals.max() - totals.min() <= 1
                if totals.max() == totals.min():
                    continue
                # the low-total pairs: a prefix of (label in the given order, workgroup, SIMD)
                pairs.sort(key=lambda p: (rank[p[0] % 8], p[0], p[1]))
                low = np.array([p[2] for p in pairs]) == totals.min()
                assert np.all(low[:-1] >= low[1:]), (frames, order)
                labels = [rank[p[0] % 8] for p, is_low in zip(pairs, low) if is_low]
                assert labels[0] == 0 and set(labels) == set(range(max(labels) + 1))


def test_the_length_multiset_differs_only_through_the_first_and_last_run():
    """Config 2: under the orders that keep tile 0 short and the last tile as it was the lengths are the even spread's multiset;
    under the others at most the first and the last run trade places with one run each (two lengths out, two in, per end)."""
    from collections import Counter
    cap = cap_of([143999], 1)
    even = cut([143999], cap, 1, None)
    its_e = iterations(even, 1)
    assert even[0] == 68 and its_e[0] == 17
    kept, moved = 0, 0
    for order in ORDERS:
        l = cut([143999], cap, 1, order)
        its = iterations(l, 1)
        a, b = Counter(l.tolist()), Counter(even.tolist())
        ends_moved = int(its[0] != its_e[0]) + int(its[-1] != its_e[-1])
        assert sum((a - b).values()) == sum((b - a).values()) <= 2 * ends_moved
        kept += ends_moved == 0
        moved += ends_moved > 0
    assert kept > 0 and moved > 0
    l = cut([143999], cap, 1, IDENTITY[::-1])          # label 0 the fastest: tile 0 long, a later run short instead
    assert l[0] == 72 and iterations(l, 1)[0] == 18


def test_config2_places_the_352_short_pairs_on_the_slow_labels():
    """The headline plan: 1 696 runs of 18 iterations and 352 of 17.  The even spread leaves a 36-iteration SIMD on every CU; under
    an order the 352 pairs of 35 fill the two slowest labels (128 pairs each) and 96 pairs of the third, whose workgroups come in
    turn, and in a pair that is low in both cuts the same member is the short one."""
    cap = cap_of([143999], 1)
    even = iterations(cut([143999], cap, 1, None), 1)
    assert sorted(np.unique(even, return_counts=True)[1].tolist()) == [352, 1696]
    per_cu = even.reshape(-1, 2, 4).sum(axis=1)
    assert np.all(per_cu.max(axis=1) == 36)
    for order in ORDERS:
        its = iterations(cut([143999], cap, 1, order), 1)
        tot = its.reshape(-1, 2, 4).sum(axis=1)                    # [workgroup][SIMD]
        label_max = [int(tot[label::8].max()) for label in range(8)]
        assert [label_max[label] for label in order] == [35, 35, 36, 36, 36, 36, 36, 36]
        low_wgs = np.nonzero((tot == 35).any(axis=1))[0]
        third = [j for j in low_wgs if j % 8 == order[2]]
        assert len(low_wgs) == 32 + 32 + 24 and third == list(range(order[2], order[2] + 8 * 24, 8))
        both = (tot == 35) & (per_cu == 35)
        assert both.any()
        a, b = its.reshape(-1, 2, 4), even.reshape(-1, 2, 4)
        assert np.array_equal(a[:, 0, :][both], b[:, 0, :][both])


def test_a_declined_plan_stays_declined():
    for frames, cap, shrink in (([1000000], 72, 1), ([20000], 72, 1), ([143999], 72, 5)):
        assert len(cut(frames, cap, shrink, None, ordered_entry=False)) == 0
        for order in ORDERS:
            assert len(cut(frames, cap, shrink, order)) == 0
