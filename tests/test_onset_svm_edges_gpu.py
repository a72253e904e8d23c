"""Edges of svm_binary_proba_kernel (pyaudioanalysis_amd/csrc/kernels_svm.hpp) through paa_svm_binary_proba_f64, against
tests/onset_svm_ref.py -- libsvm's binary probability path restated in NumPy.  -m gpu.  Needs no scikit-learn: the models
are seeded arrays (arithmetic coverage, not trained classifiers).

Covered: n_dims 1 .. 72 (the kernel's register array) and the rejected 0 / 73, n_frames around the 64-lane wave and the
256-thread block, 1 / 2 / 97 support vectors, the linear kernel with several support vectors (the Python wrapper folds
them into one, so only the C ABI reaches that loop), RBF with gamma from 1e-6 to 10, Platt slopes of both signs, scale
vectors mixing 1e-3 and 1e3, and decision values that saturate the clip to [1e-7, 1 - 1e-7] on both sides, with |fApB|
above 40 and above 750 where the unstable form of the sigmoid overflows.  Every case keeps every frame 1e-9 clear of the
early-exit threshold of multiclass_probability at every iteration (asserted on the CPU in tests/test_sim_ref_cpu.py), so
both sides take the same number of iterations and all frames are compared."""
import numpy as np
import pytest

import onset_svm_ref as R
from pyaudioanalysis_amd import _ffi, audioSegmentation

pytestmark = pytest.mark.gpu


def _call(lib, model, feats, mean, scale, n_dims=None, n_frames=None, n_sv=None, out=None):
    feats = np.ascontiguousarray(feats)
    out = np.full(feats.shape[1], -5.0) if out is None else out
    rc = lib.paa_svm_binary_proba_f64(
        _ffi.as_f64p(feats), feats.shape[0] if n_dims is None else n_dims, feats.shape[1] if n_frames is None else n_frames,
        _ffi.as_f64p(mean), _ffi.as_f64p(scale), _ffi.as_f64p(model["sv"]), _ffi.as_f64p(model["coef"]),
        model["sv"].shape[0] if n_sv is None else n_sv, model["intercept"], model["gamma"], model["prob_a"], model["prob_b"],
        _ffi.as_f64p(out))
    return rc, out


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_onset_probability_cases(gpu_lib, name):
    model, feats, mean, scale, ref, _ = R.make_case(name)
    assert ref["margin"].min() > R.MARGIN_MIN
    rc, got = _call(gpu_lib, model, feats, mean, scale)
    assert rc == 0, _ffi.last_error()
    err = np.abs(got - ref["prob1"])
    print("%s: max abs diff %.3g over %d frames, iterations %d..%d" % (name, err.max(), err.size, ref["iters"].min(),
                                                                       ref["iters"].max()))
    assert np.all(np.isfinite(got))
    assert err.max() < 1e-10, (name, int(err.argmax()), err.max())
    # a clipped pairwise probability is the same number on both sides, and the iteration is restated operation for
    # operation: those frames must agree exactly
    clipped = (ref["r01"] == R.CLIP) | (ref["r01"] == 1 - R.CLIP)
    if name.startswith("sat_"):
        assert clipped.sum() >= 100
    assert np.array_equal(got[clipped], ref["prob1"][clipped])


def test_onset_probability_argument_errors(gpu_lib):
    model, feats, mean, scale, ref, _ = R.make_case("lin_d72_f257_sv97")
    wide = np.zeros((73, feats.shape[1]))
    m73 = dict(model, sv=np.zeros((97, 73)))
    for kw in (dict(n_dims=0), dict(n_frames=0), dict(n_sv=0), dict(n_dims=-1), dict(n_frames=-1)):
        rc, out = _call(gpu_lib, model, feats, mean, scale, **kw)
        assert rc == _ffi.ERR_ARG and np.all(out == -5.0), kw
    rc, out = _call(gpu_lib, m73, wide, np.zeros(73), np.ones(73))
    assert rc == _ffi.ERR_ARG and np.all(out == -5.0)
    out = np.full(feats.shape[1], -5.0)
    f = lambda a: _ffi.as_f64p(a)
    base = [f(feats), 72, feats.shape[1], f(mean), f(scale), f(model["sv"]), f(model["coef"]), 97, model["intercept"],
            model["gamma"], model["prob_a"], model["prob_b"], f(out)]
    for k in (0, 3, 4, 5, 6, 12):
        args = list(base)
        args[k] = None
        assert gpu_lib.paa_svm_binary_proba_f64(*args) == _ffi.ERR_ARG
    assert np.all(out == -5.0)
    # and the same arguments unbroken still work
    rc, got = _call(gpu_lib, model, feats, mean, scale)
    assert rc == 0 and np.max(np.abs(got - ref["prob1"])) < 1e-10


@pytest.mark.parametrize("name", ["lin_d68_f255_sv97", "rbf_d34_f1000_sv97"])
def test_svm_onset_probability_wrapper_with_stand_in(gpu_lib, name):
    """audioSegmentation.svm_onset_probability on an object that carries the attributes it reads from an SVC.  The wrapper
    folds a linear model's support vectors into one weight vector: same value up to the rounding order of the sum."""
    model, feats, mean, scale, ref, _ = R.make_case(name)
    got = audioSegmentation.svm_onset_probability(feats, mean, scale, R.StandIn(model))
    assert got.shape == ref["prob1"].shape
    assert np.max(np.abs(got - ref["prob1"])) < 1e-10


def test_svm_onset_probability_wrapper_errors(gpu_lib):
    model, feats, mean, scale, _, _ = R.make_case("lin_d34_f64_sv97")
    with pytest.raises(NotImplementedError):
        audioSegmentation.svm_onset_probability(feats, mean, scale, R.StandIn(model, kernel="poly"))
    with pytest.raises(ValueError):
        audioSegmentation.svm_onset_probability(feats, mean, scale, R.StandIn(model, classes=(0, 1, 2)))
    with pytest.raises(ValueError):
        audioSegmentation.svm_onset_probability(feats[:33], mean, scale, R.StandIn(model))
    with pytest.raises(ValueError):
        audioSegmentation.svm_onset_probability(feats, mean[:33], scale, R.StandIn(model))
    with pytest.raises(ValueError):
        audioSegmentation.svm_onset_probability(feats, mean, scale[:33], R.StandIn(model))
    with pytest.raises(ValueError):
        audioSegmentation.svm_onset_probability(feats[0], mean, scale, R.StandIn(model))
