"""The host paths of the tree fitters -- the boosting sweep, the two forest sweeps and the builder entry points -- reproduce, bit for
bit, what they gave before they were put on shared pieces (JobClasses, TreeBatch, TreeScorer and TreeArrays of lib_treefit.hpp, the
private helpers of audioTrainTest.py): tests/golden/treefit_host_parent_bits.npz, written by
scripts/make_treefit_host_bits_golden.py in a checkout of that earlier commit; the calls and how they are run are the script's.
The kernels are the same and a tree is a function of its job alone, so equality is exact: np.array_equal on every output, with equal
shapes and dtypes; a difference is an indexing mistake of the host.  The record holds for the compiler that made it (the rule of
profiles/*_device_code.json).  The two tests about the record and the tables need no GPU."""
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


gen = _script("make_treefit_host_bits_golden")
with np.load(os.path.join(GOLDEN_DIR, "treefit_host_parent_bits.npz"), allow_pickle=False) as z:
    GOLDEN = {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def same_compiler():
    have = _script("device_code_hash").compiler_id()
    if str(GOLDEN["compiler"]) != have:
        pytest.skip("record made by %s, this host has %s" % (GOLDEN["compiler"], have))


@pytest.mark.gpu
@pytest.mark.parametrize("name", gen.call_names())
def test_outputs_equal_the_earlier_commit_bit_for_bit(gpu_lib, same_compiler, name):
    prefix = name + "."
    want = {k[len(prefix):]: v for k, v in GOLDEN.items() if k.startswith(prefix)}
    got = gen.run(name)
    assert set(got) == set(want) == set(gen.expected_keys(name))
    for key in sorted(want):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (name, key, got[key].shape, got[key].dtype)
        assert np.array_equal(got[key], want[key]), (name, key, np.argwhere(np.atleast_1d(got[key] != want[key]))[:4].tolist())
    if name.startswith("boost_"):
        chunked = name.endswith("chunked")
        assert int(got["n_chunks"]) == (gen.BOOST_CHUNKS[name.startswith("boost_trees1")] if chunked else 1)


def test_the_record_holds_every_call_and_nothing_else():
    keys = {"%s.%s" % (name, key) for name in gen.call_names() for key in gen.expected_keys(name)}
    assert keys == set(GOLDEN) - {"kind", "compiler"}
    assert str(GOLDEN["kind"]) == "treefit_host_bits"
    for trees in (True, False):                     # the chunks the earlier commit reported are the script's
        assert int(GOLDEN["boost_trees%d_chunked.n_chunks" % trees]) == gen.BOOST_CHUNKS[trees] >= 3
        assert int(GOLDEN["boost_trees%d_default.n_chunks" % trees]) == 1


def test_the_cases_cover_the_edges_of_the_shared_pieces():
    """What the record was asked to reach is in the script's tables (a table edited down would still pass above): a caller's order
    of boosting jobs that is not the stage order, a job with a class gap, an empty test list, two builder tasks on one job, training
    lists at 256 / 257 rows, at least 3 chunks under the chunk bound."""
    gen.check_coverage()
