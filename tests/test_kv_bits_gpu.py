"""svc_class_sums_kernel (+ svc_proba_kernel), svr_bank_kernel and knn_kernel reproduce, bit for bit, what they gave before
their lane split moved to kernels_kv.hpp (tests/golden/kv_parent_bits.npz, written by scripts/make_kv_bits_golden.py with
that earlier build; the cases and how they are run are the script's).  Every value is a fixed-order chain of explicit fma's
owned by one lane group, so equality is exact: np.array_equal on labels, probabilities, predictions and neighbour lists.
The record holds for the compiler that made it (the rule of profiles/*_device_code.json): another one may expand exp and
the division differently."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _script("make_kv_bits_golden")
with np.load(os.path.join(GOLDEN_DIR, "kv_parent_bits.npz"), allow_pickle=False) as z:
    GOLDEN = {k: z[k] for k in z.files}
CASES = [(name, i) for name, cases, _ in gen.FAMILIES for i in range(len(cases))]


@pytest.fixture(scope="module")
def same_compiler():
    have = _script("device_code_hash").compiler_id()
    if str(GOLDEN["compiler"]) != have:
        pytest.skip("record made by %s, this host has %s" % (GOLDEN["compiler"], have))


@pytest.mark.parametrize("family,case", CASES, ids=["%s%d" % c for c in CASES])
def test_outputs_equal_the_earlier_build_bit_for_bit(gpu_lib, same_compiler, family, case):
    run = {name: run for name, _, run in gen.FAMILIES}[family]
    got = run(GOLDEN["pool"], case)
    want = {k.split("_", 1)[1]: v for k, v in GOLDEN.items() if k.startswith("%s%d_" % (family, case))}
    assert set(got) == set(want) and want
    for key in sorted(want):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
        assert np.array_equal(got[key], want[key]), (family, case, key, np.argwhere(got[key] != want[key])[:4].tolist())


def test_the_cases_cover_the_edges_of_the_shared_pieces():
    """The sizes the record was asked to cover are in the script's tables (a table edited down would still pass above)."""
    svc, svr, knn = gen.SVC_CASES, gen.SVR_CASES, gen.KNN_CASES
    for dims, vecs, padded in (({c[2] for c in svc}, {c[4] for c in svc}, [c for c in svc if c[5] > c[4]]),
                               ({c[0] for c in svr}, {c[1] for c in svr}, [c for c in svr if c[2] > c[1] and c[3] > c[1]]),
                               ({c[0] for c in knn}, {c[1] for c in knn}, [c for c in knn if c[2] > c[1]])):
        assert dims >= {1, 8, 9, 34, 256} and vecs >= {1, 31, 32, 33, 65} and padded
    assert {(c[0], c[1]) for c in svc} == {(kernel, k) for kernel in ("rbf", "linear") for k in (2, 3, 10)}
    assert {sum(c[3]) for c in svc} >= {1, 15, 16, 17, 33} and any(0 in c[3] for c in svc)
    assert {len(c[4]) for c in svr} >= {1, 4, 5, 9} and {n for c in svr for _, n in c[4]} == {0, 1, 15, 16, 17, 40}
    assert any({k for k, _ in c[4]} == {"rbf", "linear"} for c in svr)
    assert any(len(set(c[5])) < len(c[5]) for c in svr) and any(len(set(c[5])) == len(c[5]) > 1 for c in svr)
    assert {c[3] for c in knn} >= {1, 7, 8, 9, 16, 17, 40} and {c[4] for c in knn} == {1, 3, 32} and any(c[4] > c[3] for c in knn)
    assert {c[5] for c in knn} >= {2, 9}
