#!/usr/bin/env python3
"""Write tests/golden/kv_parent_bits.npz: the outputs of svc_class_sums_kernel (+ svc_proba_kernel), svr_bank_kernel and
knn_kernel on small seeded inputs, bit for bit, from the build BEFORE the three kernels were put on kernels_kv.hpp.

Every value of these kernels is a fixed-order chain of explicit fma's owned by one lane group, so a refactor of the shared
pieces (standardise-on-load, tile copy, RBF / linear partials, group sum) must reproduce them exactly:
tests/test_kv_bits_gpu.py runs the cases below on the library under test and asserts np.array_equal.  The shapes are the
smallest at which those pieces can go wrong: dims around the 8 lanes of a group (1, 8, 9, 34, 256), vector counts around
the 32 windows of a workgroup (1, 31, 32, 33, 65), rows around the tile of 16, every kernel type, a padded device matrix.
All inputs are slices of ONE seeded pool of doubles kept in the file; models are SvcArrays / SvrArrays / Knn (no scikit-learn).

    PAA_HIP_LIBRARY=<the parent build's libpaa_hip.so> python scripts/make_kv_bits_golden.py     # on the GPU, once
"""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "kv_parent_bits.npz")
POOL = 20000
PAD = -7.0          # fill of the SVR device output beyond n_vec

# (kernel, k, n_dims, n_support per class, n_vec, ld; ld > n_vec: the device path)
SVC_CASES = [
    ("rbf", 2, 1, [1, 0], 1, 1),                                       # one support vector, a class without
    ("linear", 3, 8, [8, 0, 7], 31, 31),                               # 15: an empty class between two others
    ("rbf", 10, 9, [2, 1, 2, 1, 2, 1, 2, 1, 2, 2], 32, 32),            # 16; k = 10: a lane's second coefficient row
    ("linear", 10, 34, [1, 2, 1, 2, 3, 1, 2, 1, 2, 2], 33, 33),        # 17
    ("rbf", 3, 256, [11, 11, 11], 33, 33),                             # 33
    ("rbf", 2, 34, [16, 17], 65, 65),
    ("linear", 2, 256, [1, 0], 1, 1),
    ("rbf", 3, 9, [5, 6, 6], 33, 40),
    ("linear", 10, 8, [3, 4, 3, 4, 3, 4, 3, 3, 3, 3], 31, 36),
]
# (n_dims, n_vec, ld, ld_out, [(kernel, n_sv)], stats: model m takes the mean / std row stats[m]; equal neighbours are the
# same_prev path, also across a chunk of 4 models; ld / ld_out > n_vec: the device path)
SVR_CASES = [
    (1, 1, 1, 1, [("rbf", 1)], [0]),
    (8, 31, 31, 31, [("rbf", 0), ("linear", 15), ("rbf", 16), ("linear", 17)], [0, 1, 2, 3]),
    (9, 32, 32, 32, [("rbf", 40), ("linear", 1), ("rbf", 0), ("linear", 16), ("rbf", 17)], [0, 0, 0, 1, 1]),
    (34, 33, 33, 33, [("linear", 15), ("rbf", 16), ("rbf", 17), ("linear", 0), ("rbf", 1), ("linear", 40), ("rbf", 15),
                      ("linear", 16), ("rbf", 17)], [0] * 9),
    (256, 33, 33, 33, [("rbf", 1), ("linear", 15), ("rbf", 0), ("rbf", 16)], [0, 1, 1, 2]),
    (34, 65, 65, 65, [("linear", 40)], [0]),
    (9, 33, 40, 37, [("linear", 17), ("rbf", 16), ("rbf", 15), ("linear", 1), ("rbf", 40)], [0, 1, 1, 1, 2]),
    (256, 1, 3, 2, [("linear", 1)], [0]),
]
# (n_dims, n_vec, ld, n_train, k, n_classes; ld > n_vec: the device path, without neighbour lists).  A model of one row has one class.
KNN_CASES = [
    (1, 1, 1, 1, 1, 1),
    (8, 31, 31, 7, 3, 2),
    (9, 32, 32, 8, 32, 2),                                             # k > n_train
    (34, 33, 33, 9, 1, 9),
    (256, 33, 33, 16, 3, 2),
    (34, 65, 65, 17, 32, 9),
    (9, 65, 65, 40, 32, 9),
    (8, 32, 32, 40, 3, 9),
    (1, 33, 33, 40, 1, 2),
    (9, 33, 40, 17, 3, 9),
    (256, 1, 5, 7, 32, 2),
]


class _Pool:
    """Consecutive slices of the seeded pool, wrapping round: every array of a case is a different stretch of it."""

    def __init__(self, pool, start):
        self.pool, self.at = pool, start % pool.shape[0]

    def take(self, *shape):
        n = int(np.prod(shape))
        idx = (self.at + np.arange(n)) % self.pool.shape[0]
        self.at = (self.at + n) % self.pool.shape[0]
        return self.pool[idx].reshape(shape)

    def stats(self, n_dims):
        return 0.3 * self.take(n_dims), 0.5 + np.abs(self.take(n_dims))


@contextlib.contextmanager
def _on_device(*arrays):
    """Device copies of the arrays, freed on exit."""
    from pyaudioanalysis_amd import _ffi
    bufs = []
    try:
        for a in arrays:
            bufs.append(_ffi.DeviceBuffer.from_host(np.ascontiguousarray(a)))
        yield bufs
    finally:
        for b in bufs:
            b.free()


def run_svc(pool, i):
    from pyaudioanalysis_amd import audioTrainTest as aT
    kernel, k, n_dims, n_support, n_vec, ld = SVC_CASES[i]
    p = _Pool(pool, 1000 * i)
    n_sv, pairs = sum(n_support), k * (k - 1) // 2
    model = aT.SvcArrays(p.take(n_sv, n_dims), n_support, p.take(k - 1, n_sv), 0.2 * p.take(pairs), -1.0 - np.abs(p.take(pairs)),
                         0.1 * p.take(pairs), 1.0 / n_dims, kernel, np.arange(k) * 3 + 1)
    feats, (mean, std) = p.take(n_dims, ld), p.stats(n_dims)
    m = aT.svc_model(model)
    if ld == n_vec:
        idx, proba = m.predict(feats, mean, std)
    else:
        with _on_device(feats) as (d_feats,):
            idx, proba = m.predict_device(d_feats, ld, n_vec, mean, std)
    return {"labels": np.asarray(m.labels(idx), dtype=np.int64), "proba": proba}


def run_svr(pool, i):
    from pyaudioanalysis_amd import audioTrainTest as aT
    n_dims, n_vec, ld, ld_out, kinds, stats = SVR_CASES[i]
    p = _Pool(pool, 3000 + 1700 * i)
    models = [aT.SvrArrays(p.take(n_sv, n_dims), p.take(n_sv), p.take(1), 1.0 / n_dims if kernel == "rbf" else 0.0, kernel)
              for kernel, n_sv in kinds]
    rows = [p.stats(n_dims) for _ in range(max(stats) + 1)]
    means, stds = np.stack([rows[s][0] for s in stats]), np.stack([rows[s][1] for s in stats])
    feats = p.take(n_dims, ld)
    bank = aT.SvrBank(models, means, stds)
    if ld == n_vec:
        return {"out": bank.predict(feats)}
    with _on_device(feats, np.full((len(models), ld_out), PAD)) as (d_feats, d_out):
        bank.predict_device(d_feats, ld, n_vec, d_out, ld_out)
        return {"out": d_out.to_host(np.float64, len(models) * ld_out).reshape(len(models), ld_out)}      # the PAD columns included


def run_knn(pool, i):
    from pyaudioanalysis_amd import audioTrainTest as aT
    n_dims, n_vec, ld, n_train, k, n_classes = KNN_CASES[i]
    p = _Pool(pool, 7000 + 1300 * i)
    train = p.take(n_train, n_dims).copy()
    if n_train >= 9:
        train[5] = train[3]                                    # equal distances: the training index decides
    m = aT.knn_model(aT.Knn(train, np.arange(n_train) % n_classes, k))
    feats, (mean, std) = p.take(n_dims, ld), p.stats(n_dims)
    if ld == n_vec:
        idx, proba, nb = m.predict(feats, mean, std, neighbors=True)
        return {"labels": idx, "proba": proba, "neighbors": nb}
    with _on_device(feats) as (d_feats,):
        idx, proba = m.predict_device(d_feats, ld, n_vec, mean, std)
    return {"labels": idx, "proba": proba}


FAMILIES = (("svc", SVC_CASES, run_svc), ("svr", SVR_CASES, run_svr), ("knn", KNN_CASES, run_knn))


def run_all(pool):
    """{"<family><case>_<output>": array} of every case on the library in use."""
    out = {}
    for name, cases, run in FAMILIES:
        for i in range(len(cases)):
            for key, value in run(pool, i).items():
                out["%s%d_%s" % (name, i, key)] = value
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import device_code_hash
    pool = np.random.default_rng(20261018).standard_normal(POOL)
    arrays = run_all(pool)
    np.savez(args.out, kind=np.array("kv_bits"), pool=pool, compiler=np.array(device_code_hash.compiler_id() or ""), **arrays)
    print("%s: %d outputs, %d bytes" % (args.out, len(arrays), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
