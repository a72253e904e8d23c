"""SURVEY 8f4 on the GPU: self-similarity matrix (FP64 matrix cores) and music thumbnailing, through the C ABI,
against goldens of the unmodified reference and the NumPy oracle.  -m gpu.

Tolerances: a similarity entry is a cosine in [-1, 1] -> absolute 1e-9 when both sides start from the SAME feature
matrix; 2e-5 absolute (x filter length for the filtered matrix) when the features themselves come from the HIP
short-term path, whose parity bound is 1e-4 relative.  Arg-max positions and the grown thumbnail limits must be
identical."""
import ctypes as C

import numpy as np
import pytest

import paa_oracle as O
from conftest import golden_files, golden_id, load_golden
from pyaudioanalysis_amd import _ffi, audioSegmentation
from synth import synth_song

pytestmark = pytest.mark.gpu


def _cmp_nan(got, ref, tol, what):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN pattern differs"
    d = np.abs(np.nan_to_num(got) - np.nan_to_num(ref))
    assert d.max() <= tol, "%s: max abs diff %g > %g" % (what, d.max(), tol)


@pytest.mark.parametrize("path", golden_files("sim"), ids=golden_id)
def test_self_similarity_golden(gpu_lib, path):
    g = load_golden(path)
    S = audioSegmentation.self_similarity_matrix(g["features"])
    _cmp_nan(S, g["sim"], 1e-9, "sim")
    assert np.all(np.diag(S) == 1.0)
    assert np.array_equal(np.nan_to_num(S), np.nan_to_num(S.T)), "not bitwise symmetric"


@pytest.mark.parametrize("dims,n", [(68, 500), (34, 64), (13, 65), (5, 1), (1, 37), (136, 2049)])
def test_self_similarity_seeded(gpu_lib, dims, n):
    rng = np.random.default_rng(dims * 10007 + n)
    F = rng.standard_normal((dims, n)) * rng.uniform(0.1, 50.0, (dims, 1)) + rng.uniform(-5, 5, (dims, 1))
    if dims > 4:
        F[3] = 2.5                      # constant row: StandardScaler gives it scale 1
    ref = O.self_similarity_matrix(F)
    S = audioSegmentation.self_similarity_matrix(F)
    _cmp_nan(S, ref, 1e-9, "sim %dx%d" % (dims, n))


def test_self_similarity_large_properties(gpu_lib):
    """4096 vectors: symmetry, unit diagonal, range, and a checksum against the oracle."""
    rng = np.random.default_rng(99)
    F = rng.standard_normal((68, 4096)).cumsum(axis=1)      # correlated columns -> similarities spread over [-1, 1]
    S = audioSegmentation.self_similarity_matrix(F)
    assert np.array_equal(S, S.T)
    assert np.all(np.diag(S) == 1.0)
    assert np.all(np.abs(S) <= 1.0)
    ref = O.self_similarity_matrix(F)
    assert np.max(np.abs(S - ref)) <= 1e-9
    assert abs(S.sum() - ref.sum()) <= 1e-6 * abs(ref.sum()) + 1e-6


@pytest.mark.parametrize("n,m,step,l1,l2", [(200, 20, 0.5, 0, 1), (131, 7, 0.25, 0.1, 0.9), (64, 64, 0.5, 0, 1),
                                            (300, 33, 1.0, 0.25, 0.5), (40, 10, 0.05, 0, 1)])
def test_thumbnail_filter_seeded(gpu_lib, n, m, step, l1, l2):
    rng = np.random.default_rng(n * 31 + m)
    F = rng.standard_normal((68, n)).cumsum(axis=1)
    ref = O.thumbnail_filter(O.self_similarity_matrix(F), m, step, l1, l2)
    R = n - m + 1
    assert int(gpu_lib.paa_thumbnail_rows(n, m)) == R
    filt = np.empty((R, R))
    pos = np.zeros(2, dtype=np.int64)
    _ffi.check(gpu_lib.paa_thumbnail_f64(_ffi.as_f64p(np.ascontiguousarray(F)), 68, n, m, 5.0 / step, float(l1),
                                         float(l2), _ffi.as_f64p(filt), _ffi.as_i64p(pos)))
    _cmp_nan(filt, ref, 1e-9 * m, "filtered %d / %d" % (n, m))
    assert (int(pos[0]), int(pos[1])) == tuple(int(v) for v in np.unravel_index(ref.argmax(), ref.shape))


@pytest.mark.parametrize("path", golden_files("thumb"), ids=golden_id)
def test_music_thumbnailing_golden(gpu_lib, path):
    g = load_golden(path)
    x = synth_song(int(g["seed"]), float(g["seconds"]), int(g["fs"]))
    sw, ss, th = float(g["short_window"]), float(g["short_step"]), float(g["thumb_size"])
    # (1) matrix part alone, from the reference's own feature matrix: tight
    m = int(round(th / ss))
    R = g["filtered"].shape[0]
    filt = np.empty((R, R))
    pos = np.zeros(2, dtype=np.int64)
    F = np.ascontiguousarray(g["features"])
    _ffi.check(gpu_lib.paa_thumbnail_f64(_ffi.as_f64p(F), F.shape[0], F.shape[1], m, 5.0 / ss, float(g["limit_1"]),
                                         float(g["limit_2"]), _ffi.as_f64p(filt), _ffi.as_i64p(pos)))
    _cmp_nan(filt, g["filtered"], 1e-9 * m, "filtered (matrix part)")
    # (2) the whole function: samples -> features (HIP big-window path) -> similarity -> filter, all in HBM
    a1, a2, b1, b2, filt2 = audioSegmentation.music_thumbnailing(x, g["fs"], sw, ss, th, float(g["limit_1"]),
                                                                 float(g["limit_2"]))
    _cmp_nan(filt2, g["filtered"], 2e-5 * m, "filtered (whole function)")
    assert [a1, a2, b1, b2] == list(g["pos"])


def test_music_thumbnailing_stereo_and_errors(gpu_lib):
    x = synth_song(35, 12.0, 8000)
    st = np.stack([x, x], axis=1)                  # (R/2)+(L/2) of identical channels = the mono clip as float64
    mono = audioSegmentation.music_thumbnailing(x, 8000, 0.5, 0.25, 2.0)
    ster = audioSegmentation.music_thumbnailing(st, 8000, 0.5, 0.25, 2.0)
    assert mono[:4] == ster[:4]
    _cmp_nan(mono[4], ster[4], 1e-9, "mono against stereo")
    ref = O.music_thumbnailing(x, 8000, 0.5, 0.25, 2.0)
    assert list(mono[:4]) == list(ref[:4])
    with pytest.raises(ValueError):                # shorter than one window (ShortTermFeatures.py:684)
        audioSegmentation.music_thumbnailing(x[:2000], 8000, 0.5, 0.25, 2.0)
    with pytest.raises(ValueError):                # fewer vectors than the filter length
        audioSegmentation.music_thumbnailing(x[:16000], 8000, 0.5, 0.25, 10.0)
    with pytest.raises(ValueError):
        audioSegmentation.self_similarity_matrix(np.zeros((0, 5)))


def test_device_similarity_of_plan_output(gpu_lib):
    """paa_dev_self_similarity directly on the output of a feature plan (nothing leaves HBM in between)."""
    from synth import synth_clip
    x = synth_clip(77, 20 * 16000)
    plan = _ffi.Plan(np.array([0, len(x)], dtype=np.int64), 16000, 800, 400, deltas=True)
    T = plan.total_frames
    d_in = _ffi.DeviceBuffer.from_host(x)
    d_st = _ffi.DeviceBuffer(plan.out_doubles * 8)
    d_sim = _ffi.DeviceBuffer(T * T * 8)
    plan.execute(d_in, d_st)
    _ffi.check(gpu_lib.paa_dev_self_similarity(d_st.ptr, 68, T, T, d_sim.ptr))
    _ffi.sync()
    st = d_st.to_host(np.float64, 68 * T).reshape(68, T)
    S = d_sim.to_host(np.float64, T * T).reshape(T, T)
    _cmp_nan(S, O.self_similarity_matrix(st), 1e-9, "plan output")
    for b in (d_in, d_st, d_sim):
        b.free()
    plan.destroy()
