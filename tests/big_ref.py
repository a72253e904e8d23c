"""NumPy restatement of the HBM-pass transform (csrc/kernels_big.hpp), pass by pass, with the kernel's own index expressions:
big_load_kernel's packing, big_pass_r<R> for the radices 2, 3, 4, 5, big_pass_kernel's general branch for every other radix,
big_post_kernel's even recombination / odd magnitude.  float64 data and twiddles (the library's tables are doubles rounded from
long double, so are these); the sums of a butterfly are formed in long double where the radix is small enough for that to be cheap.

MISTAKES names four one-token slips of the general branch; stockham(..., mistake=...) makes one of them.  They exist for
tests/test_big_ref_cpu.py::test_one_token_mistakes_show_at_the_composite_windows_only, the record of why the windows of
tests/test_big_kernel_gpu.py were chosen: each slip is invisible at a prime window (one pass, Ns = 1, nb = 1, a = 1, k = 0)."""
import ctypes

import numpy as np

from pyaudioanalysis_amd import _ffi

TEMPLATED = (2, 3, 4, 5)
# twiddle step (k*a + q*nb) % Nc of the general branch: q*a for q*nb, k*nb for k*a, k*a dropped; output index
# (j-k)*R + k + q*Ns: q*nb for q*Ns
MISTAKES = ("step_q_a", "step_k_nb", "step_no_k", "out_q_nb")
LONG_SUM_MAX_RADIX = 1024          # general passes up to this radix accumulate in long double
_PI_L = np.longdouble("3.14159265358979323846264338327950288")


def plan(window):
    """-> (radices, Nc) of the library's own FFT plan for the window (paa_debug_fft_plan, host only)"""
    rad = np.zeros(32, dtype=np.int32)
    ln = ctypes.c_int32()
    n = _ffi.lib().paa_debug_fft_plan(int(window), rad.ctypes.data_as(_ffi.c_i32p), ctypes.byref(ln))
    assert 0 < n <= 32
    return [int(r) for r in rad[:n]], int(ln.value)


def big_plan(window, max_frames):
    """paa_debug_big_plan as a dict: Nc, Nf, even, passes, per_frame, C, need, wg_cap"""
    info = np.zeros(8, dtype=np.int64)
    _ffi.check(_ffi.lib().paa_debug_big_plan(int(window), int(max_frames), _ffi.as_i64p(info)))
    return dict(zip(("Nc", "Nf", "even", "passes", "per_frame", "C", "need", "wg_cap"), (int(v) for v in info)))


def twiddles(n, length=None):
    """exp(-2 pi i j / length), j < n, rounded to double from long double (tables.hpp: build_fft_plan)"""
    a = -(np.arange(n, dtype=np.longdouble) * (2 * _PI_L)) / np.longdouble(length or n)
    return np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64)


def _small_dft(v):
    """v: [R, n] -> the R-point DFT along axis 0 in natural order (dft2 .. dft5 of kernels_generic.hpp), long-double sums"""
    R = v.shape[0]
    a = -(np.outer(np.arange(R), np.arange(R)) % R).astype(np.longdouble) * (2 * _PI_L) / R
    w = (np.cos(a) + 1j * np.sin(a)).astype(np.clongdouble)
    return (w @ v.astype(np.clongdouble)).astype(np.complex128)


def _pass_templated(src, R, Ns, tw):
    Nc = len(src)
    nb = Nc // R
    tstride = Nc // (Ns * R)
    j = np.arange(nb)
    k = j % Ns
    v = np.stack([src[j + r * nb] for r in range(R)])
    if Ns > 1:
        for r in range(1, R):
            v[r] = v[r] * tw[r * k * tstride]
    v = _small_dft(v)
    j0 = (j - k) * R + k
    dst = np.full(Nc, np.nan + 0j)
    for r in range(R):
        dst[j0 + r * Ns] = v[r]
    return dst


def _pass_general(src, R, Ns, tw, mistake):
    Nc = len(src)
    nb = Nc // R
    a = Nc // (Ns * R)
    o = np.arange(Nc)
    j, q = o % nb, o // nb
    k = j % Ns
    if mistake == "step_q_a":
        step = (k * a + q * a) % Nc
    elif mistake == "step_k_nb":
        step = (k * nb + q * nb) % Nc
    elif mistake == "step_no_k":
        step = (q * nb) % Nc
    else:
        step = (k * a + q * nb) % Nc
    acc = np.zeros(Nc, dtype=np.clongdouble if R <= LONG_SUM_MAX_RADIX else np.complex128)
    idx = np.zeros(Nc, dtype=np.int64)
    for p in range(R):
        acc += src[j + p * nb] * tw[idx]
        idx += step
        idx[idx >= Nc] -= Nc
    out = (j - k) * R + k + q * (nb if mistake == "out_q_nb" else Ns)
    dst = np.full(Nc, np.nan + 0j)
    np.put(dst, out, acc.astype(np.complex128), mode="wrap")          # (a wrong output index may leave the row: wrapped, like any wrong answer)
    return dst


def stockham(z, radices, mistake=None):
    """The passes of run_big over one packed sequence z [Nc]: src -> dst with Ns = 1, R0, R0 R1, ...  -> Z [Nc] in natural order.
    mistake: one of MISTAKES, made in every general pass (the templated passes have no such expression)."""
    assert mistake is None or mistake in MISTAKES
    src = np.asarray(z, dtype=np.complex128)
    Nc = len(src)
    assert int(np.prod(np.asarray(radices, dtype=np.int64))) == Nc
    tw = twiddles(Nc)
    Ns = 1
    for R in radices:
        src = _pass_templated(src, R, Ns, tw) if R in TEMPLATED else _pass_general(src, R, Ns, tw, mistake)
        Ns *= R
    return src


def pack(frame):
    """big_load_kernel: an even window as W / 2 complex points y[2n] + i y[2n + 1], an odd one as W real points"""
    y = np.asarray(frame, dtype=np.float64)
    return y[0::2] + 1j * y[1::2] if len(y) % 2 == 0 else y + 0j


def post(Z, window):
    """big_post_kernel: |X[k]| / Nf, k < Nf = window // 2"""
    Nf, Nc = window // 2, len(Z)
    k = np.arange(Nf)
    if window % 2:
        z = Z[k]
        return np.sqrt(z.real * z.real + z.imag * z.imag) * (1.0 / Nf)
    zk = Z[k]
    zm = Z[np.where(k == 0, 0, Nc - k)]
    e = 0.5 * (zk.real + zm.real) + 0.5j * (zk.imag - zm.imag)
    o = 0.5 * (zk.imag + zm.imag) + 0.5j * (zm.real - zk.real)
    x = e + twiddles(Nc, window) * o
    return np.sqrt(x.real * x.real + x.imag * x.imag) * (1.0 / Nf)


def magnitude_spectrum(frame, mistake=None):
    """What run_big leaves in a frame's spectrum row: pack, the library's radix schedule, recombination"""
    radices, Nc = plan(len(frame))
    z = pack(frame)
    assert len(z) == Nc
    return post(stockham(z, radices, mistake), len(frame))
