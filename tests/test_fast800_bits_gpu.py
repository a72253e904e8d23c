"""The 800-sample int16 kernel (steps 400 and 800, every NW = 8 instance) gives, bit for bit, what it gave before its
issue-slot work: tests/golden/fast800_bits_parent.npz holds the input clips and the feature matrices of that earlier build,
written by scripts/make_fast800_bits_golden.py (the cases, and how each is run, are the script's).  That work only removed
instructions whose results nobody reads and moved values between lanes: no operand and no order of a rounding operation
changed, so equality is exact -- np.array_equal on the uint64 views of the doubles.  (Deltas outputs whose rows 34 .. 67 are
the column differences of rows 0 .. 33 bit for bit are kept as those 34 rows; the script's expected() rebuilds the rest.)
The record holds for the compiler that made it: other group sums of the kernel (the centroid's, the chroma variance's) owe
their bits to the compiler's choice of contracting a product into the first addition, so a failure under another compiler
says so in its message before anyone looks for a kernel bug."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _script("make_fast800_bits_golden")
with np.load(os.path.join(GOLDEN_DIR, "fast800_bits_parent.npz"), allow_pickle=False) as z:
    GOLDEN = {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", gen.CASES, ids=[gen.case_id(c) for c in gen.CASES])
def _compiler_note():
    have = _script("device_code_hash").compiler_id()
    made = str(GOLDEN["compiler"])
    return "same compiler as the record" if have == made else "COMPILER MISMATCH: record made by %s, this build by %s" % (made, have)


@pytest.mark.gpu
def test_the_build_has_the_records_compiler():
    """Reported on its own, so that a toolchain change shows as ONE failure with its reason next to the bit mismatches it causes."""
    assert _compiler_note() == "same compiler as the record"


@pytest.mark.gpu
@pytest.mark.parametrize("case", gen.CASES, ids=[gen.case_id(c) for c in gen.CASES])
def test_outputs_equal_the_earlier_build_bit_for_bit(gpu_lib, case):
    got = gen.run_case(GOLDEN, case)
    want = {k[4:]: gen.expected(v, case[3]) for k, v in GOLDEN.items() if k.startswith("out_" + gen.case_id(case))}
    assert set(got) == set(want) and want
    for key in sorted(want):
        assert got[key].shape == want[key].shape and got[key].dtype == np.float64 == want[key].dtype, key
        g, w = gen.bits(got[key]), gen.bits(want[key])
        assert np.array_equal(g, w), (key, int((g != w).sum()), np.argwhere(g != w)[:6].tolist(), _compiler_note())


def test_the_record_holds_every_case_and_its_extremes():
    """The cases the record was asked to cover are in the script's table, and the hand-made clips hold what they are there for."""
    names = {c[0] for c in gen.CASES}
    assert names >= {"noise1", "noise4", "noise5", "noise9", "noise150", "noise48", "fullscale", "zeros", "onebin", "batch"}
    combos = {(fs, s, d) for fs in (16000, 22050) for s in (400, 800) for d in (False, True)}
    assert {c[1:] for c in gen.CASES} == combos and len(gen.BATCH_FRAMES) == 8
    for name in names - {"noise150", "noise48"}:
        assert {c[1:] for c in gen.CASES if c[0] == name} == combos
    # the multi-run clip: 150 frames with deltas (two halo frames), 48 without (one): at least three runs of 16 frames either way
    assert {c[1:] for c in gen.CASES if c[0] == "noise150"} == {c for c in combos if c[2]}
    assert {c[1:] for c in gen.CASES if c[0] == "noise48"} == {c for c in combos if not c[2]}
    for case in gen.CASES:
        keys = [k for k in GOLDEN if k.startswith("out_" + gen.case_id(case))]
        assert len(keys) == (8 if case[0] == "batch" else 1), case
        for k in keys:
            assert GOLDEN[k].shape[0] in ((34, 68) if case[3] else (34,))
            assert gen.expected(GOLDEN[k], case[3]).shape[0] == (68 if case[3] else 34)
        if case[0].startswith("noise"):
            assert GOLDEN[keys[0]].shape[1] == int(case[0][5:])
    assert np.array_equal(GOLDEN["pool"], gen.make_pool())
    for name, x in gen.special_clips(GOLDEN["pool"]).items():
        assert np.array_equal(GOLDEN["in_" + name], x) and x.dtype == np.int16
    full = GOLDEN["in_fullscale"].astype(np.int64)
    chunks = full[:full.size // 40 * 40].reshape(-1, 40)
    assert (np.all(chunks == -32768, axis=1)).sum() >= 5 and int((chunks[20] ** 2).sum()) == 40 << 30      # 20 pair sums of 2^31
    zeros = GOLDEN["in_zeros"]
    for step in (400, 800):
        frames = [zeros[s:s + 800] for s in range(0, zeros.size - 799, step)]
        assert any(not f.any() for f in frames)                                         # digitally silent
        assert any(np.count_nonzero(f.reshape(10, 80).any(axis=1)) == 1 for f in frames)    # one energy block, nine exact zeros
    # "onebin": of the kept bins 0 .. 399 of every frame's 800-point transform, bin 200 alone holds energy -- and the recorded
    # spectral features say the same (a centroid at a quarter of the sampling rate, not the zeros of an empty spectrum)
    onebin = GOLDEN["in_onebin"].astype(np.float64)
    for step in (400, 800):
        for s in range(0, onebin.size - 799, step):
            power = np.abs(np.fft.rfft(onebin[s:s + 800])[:400]) ** 2
            assert power[200] > 0 and np.delete(power, 200).sum() <= 1e-20 * power[200]
    for case in gen.CASES:
        if case[0] == "onebin":
            centroid = GOLDEN["out_" + gen.case_id(case)][3]
            assert np.all(np.abs(centroid - 0.5) < 0.01), (case, centroid)
