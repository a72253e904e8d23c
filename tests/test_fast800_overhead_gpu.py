"""The 800-sample int16 kernel (kernels_fast.hpp; the four fixed-list instances: 16 kHz, steps 400 and 800, deltas off and
on) gives, bit for bit, what it gave before instructions that compute nothing were taken out of its loop (hazard waits of the
time-domain chunk loop, canonicalising copies in front of maxima, register selects of the roll-off's last five bins,
exec-masked regions around single stores).  tests/golden/fast800_overhead_parent.npz holds the input clips and the feature
matrices of the build before that work, written by scripts/make_fast800_overhead_golden.py: the signals, each chosen for one of
the places that moved, and how each is run are the script's.  No floating-point operation or operand changed, so equality
is exact -- np.array_equal on the uint64 views of the doubles.  Every case also goes to the NumPy oracle at assert_parity's
default allowances, so that "equal" cannot mean "equally wrong".  Both already held on the earlier build.  (The record holds
for the compiler that made it, as tests/test_fast800_bits_gpu.py explains; a mismatch names it.)  -m gpu."""
import importlib.util
import os

import numpy as np
import pytest

import paa_oracle as O
from conftest import GOLDEN_DIR, ROOT
from test_parity_gpu import assert_parity


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _script("make_fast800_overhead_golden")
with np.load(os.path.join(GOLDEN_DIR, "fast800_overhead_parent.npz"), allow_pickle=False) as z:
    GOLDEN = {k: z[k] for k in z.files}
IDS = [gen.case_id(c) for c in gen.CASES]
_ran = {}


def _run(case):
    """One execution per case, shared by the two tests (never modified)."""
    key = gen.case_id(case)
    if key not in _ran:
        _ran[key] = gen.run_case(GOLDEN, case)
    return _ran[key]


def _compiler_note():
    have = _script("device_code_hash").compiler_id()
    made = str(GOLDEN["compiler"])
    return "same compiler as the record" if have == made else "COMPILER MISMATCH: record made by %s, this build by %s" % (made, have)


@pytest.mark.gpu
@pytest.mark.parametrize("step,deltas", gen.COMBOS, ids=["%d_%s" % (s, "d" if d else "n") for s, d in gen.COMBOS])
def test_the_instances_are_the_fixed_list_fast800_kernels(gpu_lib, step, deltas):
    from pyaudioanalysis_amd import _ffi
    plan = _ffi.Plan(np.array([0, 4400], dtype=np.int64), gen.FS, gen.WINDOW, step, deltas=deltas)
    name = plan.kernel_name
    plan.destroy()
    assert "fast_800" in name, name


@pytest.mark.gpu
@pytest.mark.parametrize("case", gen.CASES, ids=IDS)
def test_outputs_equal_the_earlier_build_bit_for_bit(gpu_lib, case):
    got = _run(case)
    want = {k[4:]: gen.expected(v, case[3]) for k, v in GOLDEN.items() if k.startswith("out_" + gen.case_id(case) + "_")}
    assert set(got) == set(want) and want
    for key in sorted(want):
        assert got[key].shape == want[key].shape and got[key].dtype == np.float64 == want[key].dtype, key
        g, w = gen.bits(got[key]), gen.bits(want[key])
        assert np.array_equal(g, w), (key, int((g != w).sum()), np.argwhere(g != w)[:6].tolist(), _compiler_note())


@pytest.mark.gpu
@pytest.mark.parametrize("case", gen.CASES, ids=IDS)
def test_outputs_against_the_oracle(gpu_lib, case):
    got = _run(case)
    clips = gen.clips_of(GOLDEN, case)
    assert len(got) == len(clips)
    for k, x in enumerate(clips):
        ref, _ = O.feature_extraction(x, gen.FS, gen.WINDOW, case[2], case[3])
        assert_parity(got["%s_%d" % (gen.case_id(case), k)], ref, "%s clip %d" % (gen.case_id(case), k),
                      sig=(x, gen.FS, gen.WINDOW, case[2]))


def test_the_record_holds_every_case_and_its_extremes():
    """The inputs in the file are the script's, and the hand-made clips hold what they are there for."""
    made = gen.make_inputs()
    assert set(made) == {k for k in GOLDEN if k == "pool" or k.startswith("in_")}
    for k, x in made.items():
        assert x.dtype == np.int16 and np.array_equal(GOLDEN[k], x), k
    assert {c[2:] for c in gen.CASES} == {(s, d) for s in (400, 800) for d in (False, True)}
    assert {n for _, n in gen.SINGLE} == {800, 1200, 2000, 2400, 29600}
    for case in gen.CASES:
        clips = gen.clips_of(GOLDEN, case)
        for k, x in enumerate(clips):
            m = GOLDEN["out_%s_%d" % (gen.case_id(case), k)]
            assert m.shape[0] in ((34, 68) if case[3] else (34,)) and m.shape[1] == (x.size - 800) // case[2] + 1, case
    assert len(gen.clips_of(GOLDEN, ("odd", 2400, 400, False))[0]) % 2 == 1           # the second clip starts at an odd sample
    # chunk loop: a sign change at every sample, pair squares at 2^31, whole chunks of the minimum; a constant minimum clip
    alt = GOLDEN["in_alt2400"].astype(np.int64)
    assert np.all(alt[:80:2] == 32767) and np.all(alt[1:80:2] == -32768) and np.all(alt[1200:] == -32768)
    assert np.all(alt[:1200:2] >= 32767 - 255) and np.all(alt[1:1200:2] <= -32768 + 255)
    assert int((alt[1200:1240] ** 2).sum()) == 40 << 30
    assert np.all(GOLDEN["in_minimum1200"] == -32768)
    # whole and fractional clip means, with samples on the mean (its floor and ceiling)
    for name, n in gen.SINGLE:
        x = GOLDEN["in_%s%d" % (name, n)].astype(np.int64)
        if name in ("whole", "edges_whole"):
            assert x.sum() == 3 * n and (x == 3).any()
        if name in ("frac", "edges_frac"):
            assert 3 * n < x.sum() < 4 * n and (x == 3).any() and (x == 4).any()
        if name.startswith("edges"):              # the sign against the mean flips exactly at the chunk edges (but for the samples on the mean)
            s = np.sign(x - x.mean())
            flips = np.flatnonzero(s[1:] != s[:-1]) + 1
            assert set(range(40, n, 40)) <= set(flips.tolist()) and len(flips) <= n // 40 + 8
    # maxima: digitally silent frames between noise; tones whose maximum sits in a lane's bin 24 and bin 0
    sil = GOLDEN["in_silence2400"]
    assert int(sil.astype(np.int64).sum()) == 0 and sum(not sil[s:s + 800].any() for s in range(0, 1601, 400)) == 3
    # roll-off: the 90 % crossing of every tone clip is the bin the table names
    for j, (strong, k) in enumerate(gen.TONES):
        p = np.abs(np.fft.fft(GOLDEN["in_tone%d" % j].astype(np.float64) - GOLDEN["in_tone%d" % j].mean())[:400]) ** 2
        assert int(np.argmax(p)) == (k if strong is None else strong)
        assert int(np.flatnonzero(np.cumsum(p) > 0.9 * p.sum())[0]) == k, (j, strong, k)
    crossing = {k for _, k in gen.TONES}
    for lane in (0, 7, 15):
        for b in gen.LANE_BINS:
            assert 25 * lane + b in crossing or (lane == 0 and b == 0)        # (bin 0 is the mean: removed)
    assert {99, 175} <= {k for s, k in gen.TONES if s is None}
