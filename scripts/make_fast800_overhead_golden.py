#!/usr/bin/env python3
"""Write tests/golden/fast800_overhead_parent.npz: input clips of the 800-sample int16 kernel (kernels_fast.hpp, the four
fixed-list instances: 16 kHz, steps 400 and 800, deltas off and on) and the feature matrices the build BEFORE the
issue-overhead work gave for them, bit for bit.

That work takes instructions that compute nothing out of the loop -- hazard waits of the time-domain chunk loop (the four
words of a 16-byte vector run side by side), canonicalising copies in front of maxima, register selects of the roll-off's
last five bins (read from LDS instead), exec-masked regions around single stores -- and changes no floating-point operation
or operand, so tests/test_fast800_overhead_gpu.py runs the cases below on the library under test and asserts np.array_equal
on the uint64 views.  The signals are chosen for the code that moves:
  chunk loop   "alt"      +32767 / -32768 alternating: a sign change at every sample, pair squares of 2^31 - 65535 and 2^31
                          next to each other (the second half is all -32768: 20 pair sums of 2^31 per chunk), saturating
                          differences against the clip mean
               "minimum"  every sample -32768: the clamp of zb - 1 applies and every sign code is equal
               "whole" / "frac"   noise around a whole-number clip mean (3) and a fractional one (3 + a third), with samples
                          exactly on the mean (and on floor / ceil of the fractional one)
               "edges_whole" / "edges_frac"   the sign against the mean is constant inside every 40-sample chunk and flips
                          at every chunk edge, so every crossing lies between a chunk's last sample and the next one's first,
                          the frames' first samples included (the pair the frame's count leaves out)
  maxima       "silence"  noise, digital silence, the negated noise (clip mean exactly 0): frames whose maximum is 0
               tones      a frame's maximum in a lane's bin 24 (bin 99) and in a lane's bin 0 (bin 175)
  roll-off     tones      bin-centred tones (one frame each, a batch): a strong tone at bin 12 and a weaker one at bin k that
                          carries the 90 % crossing, k on the first and last bin of each of a lane's five chunks in lanes 7 and
                          15, and single tones at such bins of lane 0; every lane below the crossing's never reaches it
  stores       every clip's frame 0 (flux written as 0); the 29 600-sample clips run as several runs, whose first stored frame
               follows halo frames inside the first quad
Clip lengths: 800, 1200, 2000, 2400 and 29 600 samples (1, 2, 4, 5, 73 frames at step 400: a lone quad, partial quads, several
runs), and one two-clip plan whose second clip starts at an odd sample offset (staged without the 16-byte fetch).  Noise is
cut from ONE seeded pool kept in the file.  With deltas the kernel forms rows 34 .. 67 as differences of neighbouring columns
of rows 0 .. 33 (first column 0): where the parent's output is exactly that, only rows 0 .. 33 are kept and expected() rebuilds
the others.

    PAA_HIP_LIBRARY=<the parent build's libpaa_hip.so> python scripts/make_fast800_overhead_golden.py     # on the GPU, once
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fast800_overhead_parent.npz")
FS, WINDOW = 16000, 800
POOL = 29600
COMBOS = [(step, deltas) for step in (400, 800) for deltas in (False, True)]
# (clip name, samples); "tones" and "odd" are plans of several clips
SINGLE = [("alt", 800), ("alt", 2400), ("minimum", 1200), ("minimum", 2000), ("whole", 800), ("whole", 2000), ("frac", 1200),
          ("frac", 2400), ("edges_whole", 2400), ("edges_frac", 2000), ("edges_frac", 29600), ("silence", 2400), ("silence", 29600)]
CASES = [(name, n, step, deltas) for step, deltas in COMBOS for name, n in SINGLE + [("tones", 800), ("odd", 2400)]]
# tones: (strong bin or None, bin of the crossing).  Lane = bin // 25, chunk = bin % 25 // 5
LANE_BINS = (0, 4, 5, 9, 10, 14, 15, 19, 20, 24)           # first and last bin of each of a lane's five chunks
TONES = [(None, k) for k in (1, 4, 5, 9, 10, 14, 15, 19, 20, 24)] + [(12, 175 + b) for b in LANE_BINS] + \
        [(12, 375 + b) for b in LANE_BINS] + [(None, 99), (None, 175)]


def case_id(case):
    return "%s%d_%d_%s" % (case[0], case[1], case[2], "d" if case[3] else "n")


def make_pool():
    return np.random.default_rng(20261021).integers(-12000, 12001, size=POOL).astype(np.int16)


def with_mean(x, whole, third):
    """x (int64) shifted by whole numbers so that its mean is exactly `whole` (+ about a third when `third`), with samples
    exactly on the mean's floor and ceiling; the changes are at most a few units per sample."""
    x = x.copy()
    n = x.size
    diff = int(x.sum()) - whole * n
    q, r = divmod(diff, n)
    x -= q
    x[n - r:] -= 1                                  # sum = whole * n
    a, b = n // 3, n // 3 + 1
    for idx, val in ((a, whole), (b, whole + 1)):   # samples on the mean (and one above), paid back two places on
        x[idx + 2] += x[idx] - val
        x[idx] = val
    if third:
        x[n // 2 + 1] += n // 3 + 1                 # mean = whole + (n // 3 + 1) / n
    assert x.sum() == whole * n + ((n // 3 + 1) if third else 0) and np.abs(x).max() < 32768
    return x


def single_clip(pool, name, n):
    p = pool[:n].astype(np.int64)
    if name == "alt":
        # (a bare alternation is the Nyquist tone: the kept bins 0 .. 399 would hold round-off only, so past the first two
        # chunks the peaks carry the pool's low eight bits)
        u = p & 255
        u[:80] = 0
        x = np.where(np.arange(n) % 2 == 0, 32767 - u, -32768 + u)
        x[n // 2 // 40 * 40:] = -32768              # whole chunks of the minimum behind it
    elif name == "minimum":
        x = np.full(n, -32768)
    elif name in ("whole", "frac"):
        x = with_mean(p, 3, name == "frac")
    elif name.startswith("edges"):
        sign = np.where((np.arange(n) // 40) % 2 == 0, 1, -1)
        x = with_mean(sign * (1500 + np.abs(p) // 2), 3, name == "edges_frac")
    elif name == "silence":
        k = (n - 1600) // 2 if n <= 2400 else 12000
        x = np.concatenate([p[:k], np.zeros(n - 2 * k, dtype=np.int64), -p[:k]])
        assert x.sum() == 0
    else:
        raise ValueError(name)
    assert x.size == n
    return np.ascontiguousarray(x.astype(np.int16))


def tone_clips(pool):
    """One frame per entry of TONES, over a noise floor 35 dB below the tone (without one, every band but the tone's holds
    round-off only and the reference's own MFCCs are ill-conditioned)."""
    t = np.arange(WINDOW)
    clips = []
    for j, (strong, k) in enumerate(TONES):
        x = 9000.0 * np.cos(2 * np.pi * k * t / WINDOW + 0.3)
        if strong is not None:                      # 80 % of the energy at the strong bin, 20 % at bin k: the crossing is k
            x = 18000.0 * np.cos(2 * np.pi * strong * t / WINDOW + 0.1) + x
        x = np.round(x).astype(np.int64) + pool[37 * j:37 * j + WINDOW].astype(np.int64) // 40
        clips.append(np.ascontiguousarray(x.astype(np.int16)))
    return clips


def clips_of(inputs, case):
    """The int16 clips of a case (a list: one plan), from the arrays of the golden file."""
    name, n = case[0], case[1]
    if name == "tones":
        return [inputs["in_tone%d" % j] for j in range(len(TONES))]
    if name == "odd":                               # the second clip starts at sample 1203 of the packed buffer
        return [np.ascontiguousarray(inputs["pool"][5000:6203]), inputs["in_edges_whole2400"]]
    return [inputs["in_%s%d" % (name, n)]]


def run_case(inputs, case):
    """{"<case id>_<clip>": matrix} of one case on the library in use."""
    from pyaudioanalysis_amd import ShortTermFeatures
    clips = clips_of(inputs, case)
    if len(clips) == 1:
        out, _ = ShortTermFeatures.feature_extraction(clips[0], FS, WINDOW, case[2], case[3])
        return {case_id(case) + "_0": out}
    res, _ = ShortTermFeatures.feature_extraction_batch(clips, FS, WINDOW, case[2], case[3])
    return {"%s_%d" % (case_id(case), k): m for k, m in enumerate(res)}


def with_delta_rows(base):
    """(68, T): the 34 rows and their column differences (first column 0), as the kernel forms them."""
    return np.vstack([base, np.diff(base, axis=1, prepend=base[:, :1])])


def bits(m):
    return np.ascontiguousarray(m).view(np.uint64)


def expected(stored, deltas):
    """The full matrix of a stored output: a deltas case kept as its first 34 rows gets the other 34 back."""
    return with_delta_rows(stored) if deltas and stored.shape[0] == 34 else stored


def make_inputs():
    pool = make_pool()
    inputs = {"pool": pool}
    for name, n in SINGLE:
        inputs["in_%s%d" % (name, n)] = single_clip(pool, name, n)
    for j, x in enumerate(tone_clips(pool)):
        inputs["in_tone%d" % j] = x
    return inputs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import device_code_hash
    from pyaudioanalysis_amd import _ffi
    inputs = make_inputs()
    outputs = {}
    for case in CASES:
        plan = _ffi.Plan(np.array([0, 4400], dtype=np.int64), FS, WINDOW, case[2], deltas=case[3])
        kernel = plan.kernel_name
        plan.destroy()
        assert "fast_800" in kernel, (case, kernel)
        for key, m in run_case(inputs, case).items():
            if case[3] and np.array_equal(bits(with_delta_rows(m[:34])), bits(m)):
                m = m[:34]
            outputs["out_" + key] = np.ascontiguousarray(m)
    np.savez_compressed(args.out, kind=np.array("fast800_overhead"), compiler=np.array(device_code_hash.compiler_id() or ""),
                        **inputs, **outputs)
    print("%s: %d outputs, %d frames (%d of the deltas outputs kept whole), %d bytes" % (
        args.out, len(outputs), sum(m.shape[1] for m in outputs.values()), sum(m.shape[0] == 68 for m in outputs.values()),
        os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
