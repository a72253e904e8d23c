"""The clip statistics pass (csrc/kernels_aux.hpp: clip_stats_i16_kernel, clip_stats_stereo_kernel, clip_stats_f64_kernel) and
the clip constants formed from its partials (csrc/device_common.hpp: clip_norm_wave, run as clip_params_kernel) against exact
arithmetic, through paa_debug_plan_clip_norms: a plan plus the accessor, no feature kernel runs.  -m gpu.
(ShortTermFeatures.py:14-19, :567-570)

Reference, integer samples: s = sum(x) in Python integers (x = L + R for stereo), mean = (float(s) sc) / n, peak =
max(|max sc - mean|, |min sc - mean|), inv = 1 / (peak + 1e-10) with sc = 2^-15 (int16) / 2^-16 (stereo): every partial sum is
exact below 2^53, so this is NumPy's (np.double(x) / 2**15).mean() and np.abs(sig - mean).max() bit for bit
(tests/test_clip_stats_ref_cpu.py pins it to paa_oracle.normalize_clip) and mean, inv and every derived constant are compared
with ==.

Reference, float64 samples: math.fsum.  The kernel adds in another order, so its mean may differ by the summation bound
2 k eps sum|x| sc / n, k = the additions on the longest chain from a sample to the clip's sum.  Counted from the code:
clip_stats_f64_kernel at a chunk of L samples = L / 2 double2 vectors gives a thread ceil(L / 512) folds (one addition each onto
s or s2), one addition for a head / tail sample, s += s2, six xor-shuffle steps and two levels of the four-wave sum; clip_norm_wave
adds ceil(chunks / 64) partials per lane and six shuffle steps.  At the 4096-sample chunk of every float64 case here and the 449
chunks of the longest clip: (8 + 1 + 1 + 6 + 2) + (8 + 6) = 32 (k_of below computes it per clip).  Minimum and maximum are exact,
so peak moves by at most the mean's deviation plus the rounding of one subtraction, and inv = 1 / (peak + 1e-10) by the relative
amount bound / (peak + 1e-10) plus the roundings of the subtraction, the addition and the division: 4 eps.  The derived constants
of a float64 clip are restated from the DEVICE's mean with ==.  Observed maxima are printed (-s shows them).

Geometry (samples per chunk, chunks per clip, first chunk, CUs) is read back from the accessor; every case asserts that the
geometry it aimed at is the one it got."""
import ctypes
import functools
import math

import numpy as np
import pytest

from pyaudioanalysis_amd import _ffi

pytestmark = pytest.mark.gpu

I16, F64, STEREO = 0, 1, 2
KIND_NAME = {I16: "i16", F64: "f64", STEREO: "stereo"}
VEC = {I16: 8, STEREO: 4, F64: 2}           # samples (stereo: frames) per 16-byte vector
ITEM = {I16: 2, STEREO: 4, F64: 8}          # bytes per sample
SCALE = {I16: 2.0 ** -15, STEREO: 2.0 ** -16, F64: 2.0 ** -15}
EPS = 2.0 ** -52
FS, W = 16000, 320                            # the ct family's smallest window keeps the clips short
MIN_CHUNK, MAX_CHUNK = 4096, 131072
FIELDS = ("mean", "inv", "mu", "delta_mu", "m_int", "zb", "mu_whole", "dc_shift")
OBSERVED = {"mean": 0.0, "mean_bound": 0.0, "inv": 0.0, "inv_bound": 0.0, "k": 0}      # float64: largest deviation / its bound seen


def derived(mean, inv, window):
    """the constants clip_norm_wave derives from (mean, inv), restated (np.rint: ties to even, like nearbyint)"""
    mu = mean * 32768.0
    m_int = float(min(max(np.rint(mu), -40000.0), 40000.0))
    fl = math.floor(mu)
    return {"mean": mean, "inv": inv, "mu": mu, "delta_mu": mu - m_int, "m_int": m_int,
            "zb": float(min(max(fl, -32768.0), 32767.0)), "mu_whole": float(fl == mu), "dc_shift": 2.0 * window * (mu - m_int)}


def counts_of(sig, kind):
    """the integers the statistics are formed of (stereo: L + R)"""
    if kind == STEREO:
        return sig[:, 0].astype(np.int64) + sig[:, 1].astype(np.int64)
    return sig.astype(np.int64)


def exact_int(s, lo, hi, n, kind, window):
    sc = SCALE[kind]
    mean = (float(s) * sc) / n
    peak = max(abs(hi * sc - mean), abs(lo * sc - mean))
    return derived(mean, 1.0 / (peak + 1e-10), window)


def k_of(chunk, chunks):
    return (-(-chunk // 512) + 1 + 1 + 6 + 2) + (-(-chunks // 64) + 6)


def assert_int_clip(row, s, lo, hi, n, kind, window, what):
    assert abs(s) < 2 ** 53
    ref = exact_int(int(s), int(lo), int(hi), int(n), kind, window)
    got = dict(zip(FIELDS, row[:8]))
    bad = [f for f in FIELDS if not got[f] == ref[f]]
    assert not bad, "%s: %s" % (what, ", ".join("%s = %.17g, exact %.17g" % (f, got[f], ref[f]) for f in bad))


def assert_f64_clip(row, x, chunk, window, what):
    n, sc = len(x), SCALE[F64]
    total, sabs = math.fsum(x), float(np.abs(x).sum()) * (1.0 + 1e-9)          # (the bound itself need not be exact)
    mean = (total * sc) / n
    k = k_of(chunk, int(row[9]))
    bound = 2.0 * k * EPS * sabs * sc / n
    peak = max(abs(float(x.max()) * sc - mean), abs(float(x.min()) * sc - mean))
    inv = 1.0 / (peak + 1e-10)
    inv_bound = inv * (bound / (peak + 1e-10) + 4.0 * EPS)
    d_mean, d_inv = abs(row[0] - mean), abs(row[1] - inv)
    if d_mean >= OBSERVED["mean"]:
        OBSERVED.update(mean=d_mean, mean_bound=bound, k=k)
    if d_inv >= OBSERVED["inv"]:
        OBSERVED.update(inv=d_inv, inv_bound=inv_bound)
    assert d_mean <= bound, "%s: mean %.17g, fsum %.17g: off by %.3g, bound %.3g (k = %d)" % (what, row[0], mean, d_mean, bound, k)
    assert d_inv <= inv_bound, "%s: inv %.17g, fsum %.17g: off by %.3g, bound %.3g" % (what, row[1], inv, d_inv, inv_bound)
    ref = derived(float(row[0]), float(row[1]), window)
    bad = [f for f, g in zip(FIELDS, row[:8]) if not g == ref[f]]
    assert not bad, "%s: %s do not follow from the device's mean" % (what, bad)


def report_f64(what):
    print("%s: float64 mean off by at most %.3g (bound %.3g, k = %d), inv by %.3g (bound %.3g)"
          % (what, OBSERVED["mean"], OBSERVED["mean_bound"], OBSERVED["k"], OBSERVED["inv"], OBSERVED["inv_bound"]))


class Batch:
    """a plan over clips of the given lengths with its packed samples on the device; norms() runs the accessor"""

    def __init__(self, sigs, kind, window=W, step=W, fs=FS, mode=0, packed=None):
        self.kind, self.window = kind, window
        self.lens = [len(s) for s in sigs]
        self.offsets = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int64)
        self.plan = _ffi.Plan(self.offsets, fs, window, step, deltas=False, sample_kind=kind, mode=mode)
        packed = np.concatenate(sigs) if packed is None else packed
        self.buf = _ffi.DeviceBuffer(packed.nbytes + 64)          # (slack behind the last clip: a loop bound edited to show that these tests bite reads one vector past a chunk)
        _ffi.check(_ffi.lib().paa_memcpy_h2d(self.buf.ptr, packed.ctypes.data_as(ctypes.c_void_p), packed.nbytes))

    def norms(self):
        out = np.full(10 * (self.plan.n_clips + 1), np.nan)
        _ffi.check(_ffi.lib().paa_debug_plan_clip_norms(self.plan.handle, self.buf.ptr, _ffi.as_f64p(out), out.size))
        head, rows = out[:10], out[10:].reshape(-1, 10)
        assert head[2] == self.plan.n_clips and head[5] == self.kind and head[3] == rows[:, 9].sum()
        self.chunk, self.num_cu, self.inline = int(head[0]), int(head[1]), int(head[4])
        return rows

    def poke(self, index, value):
        """overwrite sample (stereo: frame) `index` of the packed buffer"""
        v = np.ascontiguousarray(value, dtype=np.float64 if self.kind == F64 else np.int16)
        assert v.nbytes == ITEM[self.kind]
        dst = ctypes.c_void_p(self.buf.ptr.value + int(index) * ITEM[self.kind])
        _ffi.check(_ffi.lib().paa_memcpy_h2d(dst, v.ctypes.data_as(ctypes.c_void_p), v.nbytes))

    def close(self):
        self.plan.destroy()
        self.buf.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@functools.lru_cache(maxsize=None)
def device_cus():
    with Batch([np.zeros(W, dtype=np.int16)], I16) as b:
        b.norms()
        return b.num_cu


def ripple(rng, n, kind, level):
    """a seeded ripple of +-3 counts around a level (float64: with fractions no sum of which is exact)"""
    if kind == I16:
        return (level + rng.integers(-3, 4, n)).astype(np.int16)
    if kind == STEREO:
        return (level + rng.integers(-3, 4, (n, 2))).astype(np.int16)
    return level + rng.uniform(-3.0, 3.0, n) + 0.1


def extreme(kind, level, up):
    """a sample that alone decides the peak"""
    v = level + (20011 if up else -20011)
    if kind == STEREO:
        return np.array([v, v - 7], dtype=np.int16)
    return np.float64(v + 0.3) if kind == F64 else np.int16(v)


def assert_clip(row, sig, kind, chunk, window, what):
    if kind == F64:
        assert_f64_clip(row, sig, chunk, window, what)
    else:
        c = counts_of(sig, kind)
        assert_int_clip(row, c.sum(), c.min(), c.max(), len(c), kind, window, what)


def poke_and_check(b, sigs, clip, pos, kind, up, what):
    """the extreme at sample pos of one clip: that clip against the reference; the buffer is restored afterwards"""
    sig = sigs[clip].copy()
    sig[pos] = extreme(kind, 1000, up)
    at = int(b.offsets[clip]) + pos
    b.poke(at, sig[pos])
    try:
        rows = b.norms()
        assert b.chunk == MIN_CHUNK
        assert_clip(rows[clip], sig, kind, b.chunk, b.window, "%s %s clip %d, extreme %s at %d (packed %d)"
                    % (what, KIND_NAME[kind], clip, "above" if up else "below", pos, at))
    finally:
        b.poke(at, sigs[clip][pos])


# ---- the lone extreme ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [I16, STEREO, F64], ids=lambda k: KIND_NAME[k])
def test_lone_extreme_in_every_head_tail_and_edge_vector(gpu_lib, kind):
    """Clips of 321 samples back to back start at every residue of the 16-byte vector, so heads of 0 .. V - 1 samples and tails of
    0 .. V - 1 occur; the one sample that decides the peak visits the first and the last 24 samples of every clip: the first and
    the last sample, every head and tail position, the first and the last vector of the body."""
    v = VEC[kind]
    rng = np.random.default_rng(1200 + kind)
    sigs = [ripple(rng, 321, kind, 1000) for _ in range(v + 1)]
    with Batch(sigs, kind) as b:
        rows = b.norms()
        assert b.chunk == MIN_CHUNK and np.all(rows[:, 9] == 1) and list(rows[:, 8]) == list(range(v + 1))
        assert sorted(set(int(o) % v for o in b.offsets[:-1])) == list(range(v))
        heads, tails = set(), set()
        for c, sig in enumerate(sigs):
            assert_clip(rows[c], sig, kind, b.chunk, W, "plain clip %d" % c)
            head = int(-b.offsets[c]) % v
            heads.add(head)
            tails.add((321 - head) % v)
            assert head < 24 and (321 - head) % v < 24
            for pos in list(range(24)) + list(range(321 - 24, 321)):
                for up in (True, False):
                    poke_and_check(b, sigs, c, pos, kind, up, "edge")
        assert heads == tails == set(range(v))
    if kind == F64:
        report_f64("lone extreme")


@pytest.mark.parametrize("kind", [I16, STEREO, F64], ids=lambda k: KIND_NAME[k])
def test_lone_extreme_on_either_side_of_a_chunk_boundary(gpu_lib, kind):
    """A clip of two chunks behind a clip of 320 + r samples: the chunk boundary sits at every residue r of the vector, the first
    chunk ends in a tail and the second starts with a head; the extreme visits the samples around the boundary and both ends."""
    v = VEC[kind]
    rng = np.random.default_rng(1300 + kind)
    for r in range(v):
        n2 = MIN_CHUNK + 3000 + r
        sigs = [ripple(rng, 320 + r, kind, 1000), ripple(rng, n2, kind, 1000)]
        with Batch(sigs, kind) as b:
            rows = b.norms()
            assert b.chunk == MIN_CHUNK and list(rows[:, 9]) == [1, 2] and list(rows[:, 8]) == [0, 1]
            assert int(b.offsets[1] + b.chunk) % v == r
            for c, sig in enumerate(sigs):
                assert_clip(rows[c], sig, kind, b.chunk, W, "plain clip %d" % c)
            for pos in [0, n2 - 1] + list(range(MIN_CHUNK - v - 1, MIN_CHUNK + v + 1)):
                for up in (True, False):
                    poke_and_check(b, sigs, 1, pos, kind, up, "boundary residue %d" % r)
    if kind == F64:
        report_f64("chunk boundary")


TINY_WINDOW = 2          # spectrogram plans take any window >= 2 and any clip of at least one window


@pytest.mark.parametrize("kind", [I16, STEREO, F64], ids=lambda k: KIND_NAME[k])
def test_clips_shorter_than_a_vector(gpu_lib, kind):
    """Head meets tail with no body: clips of 2 .. 7 samples (a spectrogram plan of window 2 takes them; they have no frame to
    compute, which the statistics pass does not care about), each sample in turn the extreme."""
    rng = np.random.default_rng(1400 + kind)
    sigs = [ripple(rng, n, kind, 1000) for n in (2, 3, 4, 5, 6, 7, 3, 2, 7)]
    with Batch(sigs, kind, window=TINY_WINDOW, step=1, mode=1) as b:
        rows = b.norms()
        assert b.chunk == MIN_CHUNK and np.all(rows[:, 9] == 1)
        for c, sig in enumerate(sigs):
            assert_clip(rows[c], sig, kind, b.chunk, TINY_WINDOW, "tiny clip %d" % c)
            for pos in range(len(sig)):
                for up in (True, False):
                    poke_and_check(b, sigs, c, pos, kind, up, "tiny")


# ---- the body loops -----------------------------------------------------------------------------------------------------------
LAST_VECTORS = (0, 1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025)


@pytest.mark.parametrize("kind", [I16, STEREO, F64], ids=lambda k: KIND_NAME[k])
def test_body_loop_boundaries_in_the_last_chunk(gpu_lib, kind):
    """One batch per sample type whose total gives chunks of more than 1025 vectors (4 num_cu chunks of L samples: L = 8256 for
    int16, 4160 for stereo; float64 has 2048 vectors in the smallest chunk, 4096).  Eleven clips of one full chunk plus a last
    chunk of head + V v + tail samples (tail = 3; 1 for float64), v = the vectors of its body: the four-loads-in-flight loop runs 0, 1 or 2 times for some
    threads and not for others, the single-load loop takes the rest.  The last chunk sits 700 counts above the rest and its last
    body vector holds the extreme (the tail when there is no body), so a missed vector moves both the sum and the peak.
    A filler clip brings the batch to its total."""
    v = VEC[kind]
    num_cu = device_cus()
    L = {I16: 8256, STEREO: 4160, F64: MIN_CHUNK}[kind]
    total = 4 * num_cu * L if L > MIN_CHUNK else 0
    rng = np.random.default_rng(1500 + kind)
    sigs, start, aimed = [], 0, []
    for nv in LAST_VECTORS:
        head = (-start) % v
        n = L + head + v * nv + min(3, v - 1)
        sig = ripple(rng, n, kind, 1000)
        sig[L:] += 700
        at = L + head + v * nv - 1 if nv else n - 1
        sig[at] = extreme(kind, 1700, nv % 2 == 0)
        sigs.append(sig)
        aimed.append((start + L, n - L, nv))
        start += n
    if total:
        assert start + W <= total
        sigs.append(ripple(rng, total - start, kind, -50))
    with Batch(sigs, kind) as b:
        rows = b.norms()
        assert b.num_cu == num_cu and b.chunk == L, "chunk of %d samples, aimed at %d" % (b.chunk, L)
        assert L // v > 1025
        for c, (a0, ln, nv) in enumerate(aimed):
            assert rows[c, 9] == 2
            b0 = min(-(-a0 // v) * v, a0 + ln)                # the kernel's body: [b0, b1)
            assert (a0 + ln - b0) // v == nv and a0 == b.offsets[c] + b.chunk
        for c, sig in enumerate(sigs):
            assert_clip(rows[c], sig, kind, b.chunk, W, "%d vectors in the last chunk" % aimed[c][2] if c < len(aimed) else "filler")
    if kind == F64:
        report_f64("body loops")


# ---- the fold of the chunk partials -------------------------------------------------------------------------------------------
FOLD_COUNTS = (1, 2, 63, 64, 65, 192, 193, 194, 255, 256, 257, 448, 449)
FOLD_BATCHES = ((1, 64, 193, 256, 449), (449, 2, 65, 192, 255), (63, 257, 194, 448))


def fold_clip(rng, chunks, kind, where):
    """a clip of `chunks` 4096-sample chunks (the last one 5 samples short); the chunk `where` sits 700 counts above the rest
    and holds the extreme"""
    n = chunks * MIN_CHUNK - 5
    sig = ripple(rng, n, kind, 1000)
    a = (chunks - 1) * MIN_CHUNK if where == "last" else 0
    sig[a:a + MIN_CHUNK] += 700
    sig[a + 1234] = extreme(kind, 1700, chunks % 2 == 0)
    return sig


@pytest.mark.parametrize("chunks", FOLD_COUNTS)
def test_fold_boundaries_one_clip(gpu_lib, chunks):
    """clip_norm_wave's four-loads-in-flight loop (i + 192 < stat_count) and its hand-over to the lane-strided loop, stat_first
    = 0: the one chunk that carries the level shift and the extreme is the clip's last (the partial a wrong bound drops) or its
    first; int16 and float64 (the two instances of the template)."""
    rng = np.random.default_rng(1600 + chunks)
    for kind in (I16, F64):
        for where in ("last", "first"):
            sig = fold_clip(rng, chunks, kind, where)
            with Batch([sig], kind) as b:
                rows = b.norms()
                assert b.chunk == MIN_CHUNK and rows[0, 8] == 0 and rows[0, 9] == chunks
                assert_clip(rows[0], sig, kind, b.chunk, W, "%d chunks, %s chunk marked" % (chunks, where))
    report_f64("fold, %d chunks" % chunks)


@pytest.mark.parametrize("kind", [I16, STEREO, F64], ids=lambda k: KIND_NAME[k])
def test_fold_boundaries_in_a_batch(gpu_lib, kind):
    """the same clips several to a batch: every clip after the first folds from its own stat_first.  Each batch stays below
    4 num_cu chunks of 4096 samples, where the chunk would grow."""
    num_cu = device_cus()
    rng = np.random.default_rng(1700 + kind)
    for counts in FOLD_BATCHES:
        assert sum(counts) <= 4 * num_cu
        for where in ("last", "first"):
            sigs = [fold_clip(rng, k, kind, where) for k in counts]
            with Batch(sigs, kind) as b:
                rows = b.norms()
                assert b.chunk == MIN_CHUNK and list(rows[:, 9]) == list(counts)
                assert list(rows[:, 8]) == list(np.cumsum((0,) + counts[:-1])) and rows[-1, 8] > 0
                for c, sig in enumerate(sigs):
                    assert_clip(rows[c], sig, kind, b.chunk, W, "batch %s clip %d, %s chunk marked" % (counts, c, where))
    if kind == F64:
        report_f64("fold in a batch")


# ---- the full chunk -----------------------------------------------------------------------------------------------------------
def test_full_chunks_of_full_scale_samples(gpu_lib):
    """num_cu chunks of 131072 samples on the negative rail: a thread's int32 partial sum holds 512 samples of -32768 (int16)
    or 512 frames of -65536 (stereo) = -2^25.  Then one sample at +32767.  One test, not a family: it uploads 67 MB and 134 MB
    once each and patches one sample for the second pass."""
    num_cu = device_cus()
    n = num_cu * MAX_CHUNK
    for kind in (I16, STEREO):
        lo = -32768 if kind == I16 else -65536
        packed = np.full(n if kind == I16 else (n, 2), -32768, dtype=np.int16)
        with Batch([packed], kind, packed=packed) as b:
            del packed
            rows = b.norms()
            assert b.chunk == MAX_CHUNK and rows[0, 8] == 0 and rows[0, 9] == num_cu and b.num_cu == num_cu
            assert rows[0, 0] == -1.0 and rows[0, 1] == 1e10 and rows[0, 2] == -32768.0 and rows[0, 6] == 1.0
            assert_int_clip(rows[0], lo * n, lo, lo, n, kind, W, "negative rail, %s" % KIND_NAME[kind])
            at = 77 * MAX_CHUNK + 4099
            b.poke(at, np.full(1 if kind == I16 else 2, 32767, dtype=np.int16))
            hi = 32767 if kind == I16 else 65534
            rows = b.norms()
            assert_int_clip(rows[0], lo * (n - 1) + hi, lo, hi, n, kind, W, "negative rail and one sample at +32767, %s" % KIND_NAME[kind])


# ---- the derived constants ----------------------------------------------------------------------------------------------------
def test_derived_constants_at_their_edges(gpu_lib):
    """m_int = nearbyint(mu) at ties (mu = k + 0.5, k even and odd, both signs: ties go to even), zb = floor(mu) clamped into
    int16, mu_whole, inv = 1e10 for a constant clip, mean = -1 on the negative rail, means next to a rail (x - m_int reaches
    65535).  Clips of 512 samples: every mean is exact."""
    n = 512
    half = lambda a, b: np.concatenate([np.full(n // 2, a), np.full(n // 2, b)]).astype(np.int16)      # noqa: E731
    one = lambda base, other: np.concatenate([np.full(n - 1, base), [other]]).astype(np.int16)          # noqa: E731
    named = {}
    for k in (4, 5, -5, -6, 0, -1, 32766, -32768):
        named["mu = %d + 0.5" % k] = (half(k, k + 1), k + 0.5)
    for k in (7, -7, 0, 32767, -32768):
        named["constant %d" % k] = (np.full(n, k, dtype=np.int16), float(k))
    named["mirrored around -7"] = (np.concatenate([np.arange(-256, 0), np.arange(1, 257)]).astype(np.int16) - 7, -7.0)
    named["positive rail but one sample"] = (one(32767, -32768), 32767 - 65535 / n)
    named["negative rail but one sample"] = (one(-32768, 32767), -32768 + 65535 / n)
    sigs = [s for s, _ in named.values()]
    with Batch(sigs, I16) as b:
        rows = b.norms()
        for row, (what, (sig, mu)) in zip(rows, named.items()):
            assert row[2] == mu, (what, row[2])
            assert_clip(row, sig, I16, b.chunk, W, what)
            if what.startswith("constant"):
                assert row[1] == 1e10 and row[6] == 1.0 and row[4] == mu and row[3] == 0.0
        by = dict(zip(named, rows))
        assert [by["mu = %d + 0.5" % k][4] for k in (4, 5, -5, -6, 0, -1)] == [4, 6, -4, -6, 0, 0]          # ties to even
        assert [by["mu = %d + 0.5" % k][5] for k in (4, 5, -5, -6, 0, -1)] == [4, 5, -5, -6, 0, -1]         # floor
        assert by["constant -32768"][0] == -1.0 and by["constant -32768"][5] == -32768 and by["constant 32767"][5] == 32767
        assert by["positive rail but one sample"][4] == 32639 and by["negative rail but one sample"][4] == -32640
    # stereo: mu = (sum of L + R) / (2 n) -- frames (k, k + 1) give k + 0.5; an odd total gives an odd multiple of 1 / 1024
    rng = np.random.default_rng(1800)
    odd = ripple(rng, n, STEREO, 300)
    odd[0, 0] += 1 - int(counts_of(odd, STEREO).sum()) % 2
    st = {"frames (4, 5)": np.tile(np.array([4, 5], dtype=np.int16), (n, 1)), "frames (-6, -5)": np.tile(np.array([-6, -5], dtype=np.int16), (n, 1)),
          "frames (-32768, -32768)": np.full((n, 2), -32768, dtype=np.int16), "frames (32767, 32767)": np.full((n, 2), 32767, dtype=np.int16),
          "frames (32767, 32766)": np.tile(np.array([32767, 32766], dtype=np.int16), (n, 1)), "odd total": odd,
          "L and R cancel": np.stack([ripple(rng, n, I16, 900)] * 2, axis=1) * np.array([1, -1], dtype=np.int16)}
    assert int(counts_of(odd, STEREO).sum()) % 2 == 1
    with Batch(list(st.values()), STEREO) as b:
        rows = b.norms()
        for row, (what, sig) in zip(rows, st.items()):
            assert_clip(row, sig, STEREO, b.chunk, W, what)
        by = dict(zip(st, rows))
        assert [by[k][2] for k in ("frames (4, 5)", "frames (-6, -5)", "frames (32767, 32766)")] == [4.5, -5.5, 32766.5]
        assert [by[k][4] for k in ("frames (4, 5)", "frames (-6, -5)", "frames (32767, 32766)")] == [4, -6, 32766]
        assert by["frames (-32768, -32768)"][0] == -1.0 and by["frames (-32768, -32768)"][1] == 1e10
        assert by["L and R cancel"][0] == 0.0 and by["L and R cancel"][1] == 1e10 and by["L and R cancel"][6] == 1.0
        assert by["odd total"][2] * 1024 % 2 == 1 and by["odd total"][6] == 0.0
    # float64 samples are not bound to int16: means beyond the rails meet both clamps (m_int at +-40000, zb at the int16 range)
    fl = {"constant -50000": np.full(n, -50000.0), "constant 50000.5": np.full(n, 50000.5), "constant -32768.5": np.full(n, -32768.5),
          "constant 2.5": np.full(n, 2.5), "constant -3.5": np.full(n, -3.5), "zeros": np.zeros(n)}
    with Batch(list(fl.values()), F64) as b:
        rows = b.norms()
        for row, (what, sig) in zip(rows, fl.items()):
            assert row[2] == sig[0] and row[1] == 1e10, what          # (sums of 512 equal dyadic values are exact in any order)
            assert_clip(row, sig, F64, b.chunk, W, what)
        by = dict(zip(fl, rows))
        assert (by["constant -50000"][4], by["constant -50000"][5]) == (-40000, -32768)
        assert (by["constant 50000.5"][4], by["constant 50000.5"][5]) == (40000, 32767)
        assert (by["constant -32768.5"][4], by["constant -32768.5"][5]) == (-32768, -32768)
        assert (by["constant 2.5"][4], by["constant -3.5"][4]) == (2, -4)
    with Batch([np.zeros(n, dtype=np.int16)], I16) as b:
        assert list(b.norms()[0, :8]) == [0.0, 1e10, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_the_accessor_leaves_the_plan_as_it_was(gpu_lib):
    """paa_plan_execute gives the same bits before and after the accessor ran on the plan, for a plan whose kernel folds the
    partials itself (320: ct) and one that reads clip_params_kernel's output (8000 at 8 kHz: wgr); too small a capacity is refused."""
    from synth import synth_clip
    for fs, window, name, inline in ((16000, 320, "st_ct_10x16", 1), (8000, 8000, "st_wgr_10x20x20", 0)):
        sigs = [synth_clip(1900 + i, n, fs) for i, n in enumerate((3 * window + 5, 2 * window))]
        with Batch(sigs, I16, window=window, step=window, fs=fs) as b:
            d_out = _ffi.DeviceBuffer.from_host(np.zeros(b.plan.out_doubles))
            b.plan.execute(b.buf, d_out)
            first = d_out.to_host(np.float64, b.plan.out_doubles)
            rows = b.norms()
            assert b.plan.kernel_name == name and b.inline == inline
            for c, sig in enumerate(sigs):
                assert_clip(rows[c], sig, I16, b.chunk, window, "window %d clip %d" % (window, c))
            out = np.zeros(29)
            assert _ffi.lib().paa_debug_plan_clip_norms(b.plan.handle, b.buf.ptr, _ffi.as_f64p(out), 29) == _ffi.ERR_ARG
            b.plan.execute(b.buf, d_out)
            assert d_out.to_host(np.float64, b.plan.out_doubles).tobytes() == first.tobytes()
            d_out.free()
