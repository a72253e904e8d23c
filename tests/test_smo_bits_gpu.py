"""smo_kernel, svr_smo_kernel and svr_smo_cached_kernel reproduce, bit for bit, what they gave before the two-variable update,
calculate_rho and the set-up of a task moved into the solver core of kernels_smo_core.hpp (tests/golden/smo_parent_bits.npz, written
by scripts/make_smo_bits_golden.py with that earlier build; the calls and how they are run are the script's).  An iteration reads
nothing but (alpha, G), the selections are exact and every sum has a fixed order, so equality is exact under every launch budget:
np.array_equal on alpha_y / beta, rho, the gap, the iteration counts, the status words, n_sv and the training predictions.
The record holds for the compiler that made it (the rule of profiles/*_device_code.json): another one may contract other
multiply-adds and expand the division differently.  The two tests about the record and the tables need no GPU."""
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


gen = _script("make_smo_bits_golden")
with np.load(os.path.join(GOLDEN_DIR, "smo_parent_bits.npz"), allow_pickle=False) as z:
    GOLDEN = {k: z[k] for k in z.files}
CALLS = {call.name: call for call in gen.calls()}


@pytest.fixture(scope="module")
def same_compiler():
    have = _script("device_code_hash").compiler_id()
    if str(GOLDEN["compiler"]) != have:
        pytest.skip("record made by %s, this host has %s" % (GOLDEN["compiler"], have))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_outputs_equal_the_earlier_build_bit_for_bit(gpu_lib, same_compiler, name):
    call = CALLS[name]
    for suffix, kw in gen.entry_points(call):
        prefix = "%s%s." % (name, suffix)
        want = {k[len(prefix):]: v for k, v in GOLDEN.items() if k.startswith(prefix)}
        assert set(want) == set(gen.SVC_OUTPUTS if call.family == "svc" else gen.SVR_OUTPUTS)
        for budget in gen.BUDGETS:
            got = gen.run(call, budget, **kw)
            assert set(got) == set(want)
            for key in sorted(want):
                assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (prefix, budget, key)
                assert np.array_equal(got[key], want[key]), (prefix, budget, key, np.argwhere(got[key] != want[key])[:4].tolist())


def test_the_record_holds_every_call_and_nothing_else():
    keys = {"%s%s.%s" % (call.name, suffix, out) for call in gen.calls() for suffix, _ in gen.entry_points(call)
            for out in (gen.SVC_OUTPUTS if call.family == "svc" else gen.SVR_OUTPUTS)}
    assert keys == set(GOLDEN) - {"kind", "compiler"}


def test_the_cases_cover_the_edges_of_the_shared_pieces():
    """What the record was asked to reach is in the script's tables (a table edited down would still pass above): on the CPU
    restatements, every clip of the update and the unclipped step of either branch, the clamp of eta, rho with free variables and
    with none, both stops; the row counts at the ownership edges, the dims, both kernels, a small and a large C, several tasks in
    one call, the three launch budgets."""
    gen.check_coverage()
