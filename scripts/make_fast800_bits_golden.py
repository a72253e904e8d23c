#!/usr/bin/env python3
"""Write tests/golden/fast800_bits_parent.npz: input clips of the 800-sample int16 kernel (kernels_fast.hpp, steps 400 and
800) and the feature matrices the build BEFORE the issue-slot work gave for them, bit for bit.

That work (64-bit integer chunk sums, shared fast_log2 / fast_div / fast_sqrt calls, reduce-to-one-lane, row_newbcast) removes
instructions whose results nobody reads and moves values between lanes; it changes no operand and no order of any rounding
operation, so tests/test_fast800_bits_gpu.py runs the cases below on the library under test and asserts np.array_equal on
the uint64 views.  The cases are the smallest at which those items can go wrong:
  * noise clips of 1, 4, 5, 9 frames (less than a quad, one quad, a quad and one frame, three quads), of 150 frames with
    deltas and of 48 frames without (several runs each, so quads that begin with two / one halo frames);
  * steps 400 and 800, with and without deltas, at 16 kHz (compile-time mel / chroma lists) and 22 050 Hz (run-time lists);
  * "fullscale": noise with whole 40-sample chunks of -32768 (20 pair sums of 2^31 in one chunk's sum of squares);
  * "zeros": digital silence (every entropy term 0 / eps) with one +A / -A pair inside it (one non-zero 80-sample energy
    block, nine exact zeros) between noise and its negated copy (the clip mean is exactly 0);
  * "onebin": +A +A -A -A repeating -- a square wave of period 4 has odd harmonics only, 200 and 600 of the 800-point transform,
    so bin 200 alone of the kept bins 0 .. 399 holds energy: one spectral-entropy quotient near 1 beside nine (near) zeros,
    and nothing but rounding in the top 25 bins (where the row's last scan entry need not be its largest);
  * eight short clips of unequal length in one plan (clips that start at odd sample offsets of the packed buffer).
Noise clips are slices of ONE seeded pool kept in the file (repeated end to end where a clip is longer than the pool: its
length is no multiple of the steps, so no two frames repeat).  With deltas the kernel forms rows 34 .. 67 as differences of
neighbouring columns of rows 0 .. 33 (first column 0): where the parent's output is exactly that, only rows 0 .. 33 are
kept and expected() rebuilds the others.

    PAA_HIP_LIBRARY=<the parent build's libpaa_hip.so> python scripts/make_fast800_bits_golden.py     # on the GPU, once
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fast800_bits_parent.npz")
WINDOW = 800
POOL = 20011                            # samples of the noise pool
NOISE_FRAMES = (1, 4, 5, 9)
LONG_FRAMES = {True: 150, False: 48}    # the multi-run clip with / without deltas (runs are at least 16 frames long)
BATCH_FRAMES = (1, 4, 5, 9, 2, 3, 6, 7)
SPECIAL = ("fullscale", "zeros", "onebin")
COMBOS = [(fs, step, deltas) for fs in (16000, 22050) for step in (400, 800) for deltas in (False, True)]
# every case: (clip name, fs, step, deltas); "batch" is the eight clips in one plan
CASES = [(name, fs, step, deltas) for fs, step, deltas in COMBOS
         for name in ["noise%d" % t for t in NOISE_FRAMES + (LONG_FRAMES[deltas],)] + list(SPECIAL) + ["batch"]]


def case_id(case):
    return "%s_%d_%d_%s" % (case[0], case[1], case[2], "d" if case[3] else "n")


def samples(frames, step):
    return WINDOW + (frames - 1) * step


def make_pool():
    return np.random.default_rng(20261019).integers(-12000, 12001, size=POOL).astype(np.int16)


def special_clips(pool):
    """The hand-made clips (kept in the file as they are), 13 frames at step 400 / 7 at step 800 at the most."""
    full = pool[1000:1000 + samples(9, 400)].copy()
    full[800:840] = -32768                       # one whole chunk
    full[1200:1320] = -32768                     # three in a row: two of them share an 80-sample energy block
    full[2000:2040] = -32768
    full[2079] = -32768                          # and a lone sample in the chunk after
    noise = pool[5000:6600]
    zeros = np.concatenate([noise, np.zeros(2400, dtype=np.int16), -noise])
    zeros[1600 + 1300] = 9000                    # the only non-zero block of the frames that lie inside the silence
    zeros[1600 + 1301] = -9000
    assert int(zeros.astype(np.int64).sum()) == 0
    onebin = np.tile(np.array([12345, 12345, -12345, -12345], dtype=np.int16), samples(9, 400) // 4)
    return {"fullscale": full, "zeros": zeros, "onebin": onebin}


def clip(inputs, name, step):
    """The int16 samples of a named clip at this step, from the arrays of the golden file."""
    if name.startswith("noise"):
        frames = int(name[5:])
        return np.resize(np.roll(inputs["pool"], -37 * frames), samples(frames, step))
    return inputs["in_" + name]


def batch_clips(inputs, step):
    return [np.ascontiguousarray(np.resize(np.roll(inputs["pool"], -211 * (k + 1)), samples(t, step) + 3 * k))      # lengths 3 k past whole frames
            for k, t in enumerate(BATCH_FRAMES)]


def run_case(inputs, case):
    """{"<case id>" or "<case id>_<clip>": matrix} of one case on the library in use."""
    from pyaudioanalysis_amd import ShortTermFeatures
    name, fs, step, deltas = case
    if name == "batch":
        res, _ = ShortTermFeatures.feature_extraction_batch(batch_clips(inputs, step), fs, WINDOW, step, deltas)
        return {"%s_%d" % (case_id(case), k): m for k, m in enumerate(res)}
    out, _ = ShortTermFeatures.feature_extraction(np.ascontiguousarray(clip(inputs, name, step)), fs, WINDOW, step, deltas)
    return {case_id(case): out}


def with_delta_rows(base):
    """(68, T): the 34 rows and their column differences (first column 0), as the kernel forms them."""
    return np.vstack([base, np.diff(base, axis=1, prepend=base[:, :1])])


def bits(m):
    return np.ascontiguousarray(m).view(np.uint64)


def expected(stored, deltas):
    """The full matrix of a stored output: a deltas case kept as its first 34 rows gets the other 34 back."""
    return with_delta_rows(stored) if deltas and stored.shape[0] == 34 else stored


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import device_code_hash
    from pyaudioanalysis_amd import _ffi
    pool = make_pool()
    inputs = {"pool": pool}
    inputs.update({"in_" + k: v for k, v in special_clips(pool).items()})
    outputs = {}
    for case in CASES:
        plan = _ffi.Plan(np.array([0, samples(9, case[2])], dtype=np.int64), case[1], WINDOW, case[2], deltas=case[3])
        kernel = plan.kernel_name
        plan.destroy()
        assert "fast_800" in kernel, (case, kernel)
        for key, m in run_case(inputs, case).items():
            if case[3] and np.array_equal(bits(with_delta_rows(m[:34])), bits(m)):
                m = m[:34]
            outputs["out_" + key] = np.ascontiguousarray(m)
    np.savez_compressed(args.out, kind=np.array("fast800_bits"), compiler=np.array(device_code_hash.compiler_id() or ""),
                        **inputs, **outputs)
    print("%s: %d outputs (%d of the deltas outputs kept whole), %d bytes" % (
        args.out, len(outputs), sum(m.shape[0] == 68 for m in outputs.values()), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
