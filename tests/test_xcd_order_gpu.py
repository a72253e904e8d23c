"""Placement of the 800-sample kernel's short runs by XCD (csrc/lib_xcd_order.hpp) on the device.  -m gpu.

The smallest balanced shape with both run lengths: one int16 clip of 40 000 frames makes 256 x 8 runs of 5 or 6 iterations.  Which
run is long and which is short is a tiling choice and the kernel's output does not depend on the tiling, so every comparison is
np.array_equal on the uint64 views of the doubles against the output of the even spread (PAA_XCD_ORDER=0: the cut without any
order).  What those bits are is pinned elsewhere (tests/test_fast800_bits_gpu.py, the parity tests); here equal bits are the whole
claim."""
import ctypes

import numpy as np
import pytest

from pyaudioanalysis_amd import _ffi

FS, WINDOW, FRAMES = 16000, 800, 40000
COMBOS = [(step, deltas) for step in (400, 800) for deltas in (False, True)]
IDS = ["%d_%s" % (step, "d" if deltas else "n") for step, deltas in COMBOS]
ORDERS = {"identity": list(range(8)), "reverse": list(range(8))[::-1], "shuffled": [3, 5, 1, 7, 0, 4, 2, 6]}
_POOL = np.random.default_rng(20261021).integers(-12000, 12001, size=700001).astype(np.int16)
_cache = {}


def samples(step):
    return WINDOW + (FRAMES - 1) * step


def device_samples():
    """The samples of the longer clip (step 800) on the device, once; the step-400 clip is their head."""
    if "x" not in _cache:
        _cache["x"] = _ffi.DeviceBuffer.from_host(np.resize(_POOL, samples(800)))
    return _cache["x"]


def force(order):
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32).ctypes.data_as(_ffi.c_i32p)
    _ffi.check(_ffi.lib().paa_debug_xcd_force_order(o))


def state():
    epoch = ctypes.c_uint64()
    order = np.zeros(8, dtype=np.int32)
    flags = _ffi.lib().paa_debug_xcd_state(_ffi.as_i32p(order), None, ctypes.byref(epoch))
    return flags, order.tolist(), epoch.value


def plan_runs(plan):
    lens = np.zeros(4096, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    epoch = ctypes.c_uint64()
    n = _ffi.check(_ffi.lib().paa_debug_plan_runs(plan.handle, _ffi.as_i32p(lens), len(lens), _ffi.as_i32p(info), ctypes.byref(epoch)))
    return lens[:n].copy(), info.tolist(), epoch.value


def host_cut(plan, info, order):
    frames = np.array([plan.total_frames], dtype=np.int64)
    out = np.zeros(4096, dtype=np.int32)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32).ctypes.data_as(_ffi.c_i32p)
    run, quantum, shrink, wg_runs, min_run, num_cu = info[:6]
    n = _ffi.lib().paa_debug_balanced_runs_ordered(_ffi.as_i64p(frames), 1, run, quantum, shrink, wg_runs, num_cu, min_run, o,
                                                   _ffi.as_i32p(out), len(out))
    assert n > 0
    return out[:n].copy()


def run_bits(plan, d_out):
    plan.execute(device_samples(), d_out)
    _ffi.sync()
    return d_out.to_host(np.float64, plan.out_doubles).view(np.uint64).copy()


@pytest.fixture
def plan_and_reference(gpu_lib, monkeypatch, request):
    """A plan of the shape, its output buffer, and the output and run lengths of the cut without any order."""
    step, deltas = request.param
    force(None)
    monkeypatch.setenv("PAA_XCD_ORDER", "0")
    plan = _ffi.Plan(np.array([0, samples(step)], dtype=np.int64), FS, WINDOW, step, deltas=deltas)
    assert "fast_800" in plan.kernel_name and plan.total_frames == FRAMES
    d_out = _ffi.DeviceBuffer(plan.out_doubles * 8)
    want = run_bits(plan, d_out)
    even, info, epoch = plan_runs(plan)
    assert epoch == 0 and len(even) == info[3] * info[5] == 2048
    monkeypatch.delenv("PAA_XCD_ORDER")
    yield plan, d_out, want, even, info
    force(None)
    plan.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("plan_and_reference", COMBOS, ids=IDS, indirect=True)
def test_switched_off_gives_the_even_spread(plan_and_reference, monkeypatch):
    """PAA_XCD_ORDER=0: the run lengths are those of balanced_runs without an order, whatever is forced."""
    plan, d_out, want, even, info = plan_and_reference
    assert np.array_equal(even, host_cut(plan, info, None))
    shrink = info[2]
    its = (even + np.where(np.arange(len(even)) > 0, shrink, 0) + 3) // 4
    assert sorted(set(its.tolist())) == [5, 6]
    force(ORDERS["shuffled"])
    monkeypatch.setenv("PAA_XCD_ORDER", "0")
    assert state()[0] & 1 == 0
    lens, _, epoch = plan_runs(plan)
    assert epoch == 0 and np.array_equal(lens, even)
    assert np.array_equal(run_bits(plan, d_out), want)


@pytest.mark.gpu
@pytest.mark.parametrize("plan_and_reference", COMBOS, ids=IDS, indirect=True)
def test_forced_orders_move_runs_not_bits(plan_and_reference):
    """Identity, reverse and a shuffled order, forced between executes of ONE plan (the lazy re-cut at execute: the epoch and the run
    lengths change, the bits do not) and on a plan created under the order."""
    plan, d_out, want, even, info = plan_and_reference
    mapped = not (state()[0] & 2)          # (a device that maps labels to XCDs differently ignores every order)
    last_epoch = 0
    for name, order in ORDERS.items():
        force(order)
        lens, _, epoch = plan_runs(plan)
        if mapped:
            assert epoch > last_epoch, name
            assert np.array_equal(lens, host_cut(plan, info, order)), name
            assert not np.array_equal(lens, even), name
        else:
            assert epoch == 0 and np.array_equal(lens, even)
        last_epoch = epoch
        got = run_bits(plan, d_out)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        lens_after, _, epoch_after = plan_runs(plan)
        assert epoch_after == epoch and np.array_equal(lens_after, lens)
    fresh = _ffi.Plan(plan.offsets, FS, WINDOW, plan_step(plan), deltas=plan.F == 68)
    try:
        lens, _, _ = plan_runs(fresh)
        assert np.array_equal(lens, host_cut(fresh, info, ORDERS["shuffled"]) if mapped else even)
        got = run_bits(fresh, d_out)
        assert np.array_equal(got, want), int((got != want).sum())
    finally:
        fresh.destroy()
    force(None)
    got = run_bits(plan, d_out)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_a_plan_with_fewer_runs_than_wave_slots_probes_and_calibration_stays_on(gpu_lib, monkeypatch):
    """Three clips of 11 000, 16 000 and 13 000 frames are cut into 2 047 runs: 256 workgroups, the last one a wave short.  That is
    a grid the calibration accepts: a forced probe launch and the device's own probes (one execute in 256 at the latest) of this
    plan leave the calibration switched on, and its output does not depend on the order either."""
    force(None)
    on_before = not (state()[0] & 2)
    frames = [11000, 16000, 13000]
    offsets = np.concatenate([[0], np.cumsum([samples_of(t, 400) for t in frames])]).astype(np.int64)
    assert offsets[-1] <= samples(800)
    monkeypatch.setenv("PAA_XCD_ORDER", "0")
    plan = _ffi.Plan(offsets, FS, WINDOW, 400, deltas=False)
    d_out = _ffi.DeviceBuffer(plan.out_doubles * 8)
    try:
        want = run_bits(plan, d_out)
        even, info, _ = plan_runs(plan)
        assert len(even) == 2047 < info[3] * info[5] and (len(even) + info[3] - 1) // info[3] == info[5] == 256
        monkeypatch.delenv("PAA_XCD_ORDER")
        rec = np.zeros(2 * 2048, dtype=np.uint64)
        n = _ffi.check(_ffi.lib().paa_debug_plan_probe(plan.handle, device_samples().ptr, d_out.ptr,
                                                       rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 2048))
        assert n == 2047
        entry, exit_ = rec[0:2 * n:2], rec[1:2 * n:2] & np.uint64((1 << 60) - 1)
        assert np.all(entry > 0) and np.all(exit_ > entry) and not rec[2 * n:].any()
        xcc = (rec[1:2 * n:2] >> np.uint64(60)).astype(np.int64)
        label = (np.arange(n) // info[3]) % 8
        if all(len(set(xcc[label == k].tolist())) == 1 for k in range(8)):
            assert not (state()[0] & 2)
        for _ in range(2):                      # the device's own probes: at least one of these executes is one, the next reads it
            for _ in range(260):
                plan.execute(device_samples(), d_out)
            _ffi.sync()
        plan.execute(device_samples(), d_out)
        _ffi.sync()
        assert (not (state()[0] & 2)) == on_before
        force(ORDERS["shuffled"])
        got = run_bits(plan, d_out)
        assert np.array_equal(got, want), int((got != want).sum())
    finally:
        force(None)
        plan.destroy()


def samples_of(frames, step):
    return WINDOW + (frames - 1) * step


def plan_step(plan):
    return (int(plan.offsets[1]) - WINDOW) // (FRAMES - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("plan_and_reference", COMBOS, ids=IDS, indirect=True)
def test_one_probe_launch(plan_and_reference):
    """2 048 records with exit after entry; every label on one XCC id with 32 workgroups each -- or the calibration has switched
    itself off.  The probe launch stores the same bits as any other."""
    plan, d_out, want, even, info = plan_and_reference
    rec = np.zeros(2 * 2048, dtype=np.uint64)
    n = _ffi.check(_ffi.lib().paa_debug_plan_probe(plan.handle, device_samples().ptr, d_out.ptr,
                                                   rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 2048))
    assert n == 2048
    got = d_out.to_host(np.float64, plan.out_doubles).view(np.uint64)
    assert np.array_equal(got, want)
    entry, exit_ = rec[0::2], rec[1::2] & np.uint64((1 << 60) - 1)
    xcc = (rec[1::2] >> np.uint64(60)).astype(np.int64)
    assert np.all(entry > 0) and np.all(exit_ > entry)
    assert int(exit_.max() - entry.min()) < 100_000_000          # (100 MHz ticks: one launch, well under a second)
    wg_runs = info[3]
    label = (np.arange(2048) // wg_runs) % 8
    one_xcd_each = all(len(set(xcc[label == k].tolist())) == 1 for k in range(8))
    if one_xcd_each:
        assert not (state()[0] & 2)
        for k in range(8):
            assert int((label == k).sum()) == 32 * wg_runs
    else:
        assert state()[0] & 2
