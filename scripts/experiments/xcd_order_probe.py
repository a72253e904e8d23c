#!/usr/bin/env python3
"""Per-label end times of the headline plan's launches, from the kernel's own probe (csrc/lib_xcd_order.hpp), and what the
placement of the short runs on the slow XCDs predicts and gives.

    python scripts/experiments/xcd_order_probe.py [--launches 20] [--between 30]

Phase A runs with PAA_XCD_ORDER=0 (the even spread, no calibration): `--launches` probe launches, `--between` plain executes in
front of each so that the chip is under load, all queued back to back.  Per launch: the end of each label's last wave in us after
the launch's first wave entered (label = workgroup mod 8), then the averages, the time per iteration tau = t / n (n = the label's
largest SIMD total: 36 everywhere under the even spread) and what the ordered cut would give: max over labels of tau x n'.
Phase B switches the calibration on, lets the library find its order by itself (executes in batches, as bench.py's pre-warm
does), prints the state and repeats the probe launches under that order.  Output goes to profiles/r13_fast800_xcd_order_probe.txt.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pyaudioanalysis_amd import _ffi          # noqa: E402

FS, WINDOW, STEP = 16000, 800, 400


def plan_runs(plan):
    lens = np.zeros(4096, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    epoch = ctypes.c_uint64()
    n = _ffi.check(_ffi.lib().paa_debug_plan_runs(plan.handle, _ffi.as_i32p(lens), len(lens), _ffi.as_i32p(info), ctypes.byref(epoch)))
    return lens[:n].copy(), info.tolist(), epoch.value


def label_totals(lens, info):
    quantum, shrink, wg_runs = info[1], info[2], info[3]
    its = (lens + np.where(np.arange(len(lens)) > 0, shrink, 0) + quantum - 1) // quantum
    simd = its.reshape(-1, wg_runs // 4, 4).sum(axis=1)          # [workgroup][SIMD]
    return np.array([int(simd[k::8].max()) for k in range(8)])


def ordered_totals(plan, info, order):
    frames = np.array([plan.total_frames], dtype=np.int64)
    out = np.zeros(4096, dtype=np.int32)
    run, quantum, shrink, wg_runs, min_run, num_cu = info[:6]
    n = _ffi.lib().paa_debug_balanced_runs_ordered(_ffi.as_i64p(frames), 1, run, quantum, shrink, wg_runs, num_cu, min_run,
                                                   np.ascontiguousarray(order, dtype=np.int32).ctypes.data_as(_ffi.c_i32p),
                                                   _ffi.as_i32p(out), len(out))
    return label_totals(out[:n], info)


def state():
    epoch = ctypes.c_uint64()
    order = np.zeros(8, dtype=np.int32)
    tau = np.zeros(8)
    flags = _ffi.lib().paa_debug_xcd_state(_ffi.as_i32p(order), _ffi.as_f64p(tau), ctypes.byref(epoch))
    return flags, order.tolist(), tau, epoch.value


def probes(plan, d_x, d_out, launches, between, info):
    rec = np.zeros(2 * 2048, dtype=np.uint64)
    rows = []
    for _ in range(launches):
        for _ in range(between):
            plan.execute(d_x, d_out)
        n = _ffi.check(_ffi.lib().paa_debug_plan_probe(plan.handle, d_x.ptr, d_out.ptr,
                                                       rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 2048))
        assert n == 2048, n
        entry, exit_ = rec[0::2].astype(np.int64), (rec[1::2] & np.uint64((1 << 60) - 1)).astype(np.int64)
        xcc = (rec[1::2] >> np.uint64(60)).astype(np.int64)
        label = (np.arange(2048) // info[3]) % 8
        rows.append(([(exit_[label == k].max() - entry.min()) / 100.0 for k in range(8)],
                     ["/".join(str(v) for v in sorted(set(xcc[label == k].tolist()))) for k in range(8)]))
    _ffi.sync()
    return rows


def table(rows, n_label):
    print("launch  " + "  ".join("label%d" % k for k in range(8)) + "   last   (us; XCC ids of the labels: %s)" % " ".join(rows[0][1]))
    for i, (t, _) in enumerate(rows):
        print("%4d    " % (i + 1) + "  ".join("%6.1f" % v for v in t) + "  %6.1f" % max(t))
    t = np.array([r[0] for r in rows])
    print("mean    " + "  ".join("%6.1f" % v for v in t.mean(axis=0)) + "  %6.1f  (mean of the launches' ends)" % t.max(axis=1).mean())
    print("n       " + "  ".join("%6d" % v for v in n_label))
    tau = t.mean(axis=0) / n_label
    print("tau     " + "  ".join("%6.3f" % v for v in tau) + "   (us per iteration)")
    return t, tau


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--between", type=int, default=30)
    args = ap.parse_args()
    _ffi.init(0)
    n = int(3600 * FS)
    x = np.resize(np.random.default_rng(2).integers(-12000, 12001, size=1000003).astype(np.int16), n)
    d_x = _ffi.DeviceBuffer.from_host(x)

    os.environ["PAA_XCD_ORDER"] = "0"
    plan = _ffi.Plan(np.array([0, n], dtype=np.int64), FS, WINDOW, STEP, deltas=False)
    d_out = _ffi.DeviceBuffer(plan.out_doubles * 8)
    for _ in range(600):                                         # (the engine clock ramps over the first 0.1 s)
        plan.execute(d_x, d_out)
    _ffi.sync()
    lens, info, epoch = plan_runs(plan)
    n_even = label_totals(lens, info)
    print("# phase A: PAA_XCD_ORDER=0, %s, %d frames, %d runs, epoch %d" % (plan.kernel_name, plan.total_frames, len(lens), epoch))
    t, tau = table(probes(plan, d_x, d_out, args.launches, args.between, info), n_even)
    order = [int(k) for k in np.argsort(-tau, kind="stable")]
    n_ord = ordered_totals(plan, info, order)
    now, then = (tau * n_even).max(), (tau * n_ord).max()
    print("order by tau, slowest first: %s; n' = %s" % (order, n_ord.tolist()))
    print("rung 1 predicts: launch end %.1f -> %.1f us (%.2f %%); per launch: %s" % (
        now, then, 100.0 * (then / now - 1.0),
        " ".join("%.2f" % (100.0 * ((tl / n_even * n_ord).max() / tl.max() - 1.0)) for tl in t)))

    del os.environ["PAA_XCD_ORDER"]
    for _ in range(40):                                          # batches with a wait, as bench.py's pre-warm
        for _ in range(20):
            plan.execute(d_x, d_out)
        _ffi.sync()
    flags, order_b, tau_b, epoch_b = state()
    lens, info, epoch = plan_runs(plan)
    print("\n# phase B: calibration on; after 800 executes: flags %d, order in force %s, epoch %d, tau %s ticks" % (
        flags, order_b, epoch_b, " ".join("%.1f" % v for v in tau_b)))
    n_b = label_totals(lens, info)
    t_b, _ = table(probes(plan, d_x, d_out, args.launches, args.between, info), n_b)
    print("mean launch end: %.1f us under the even spread, %.1f us under the order (%.2f %%)" % (
        t.max(axis=1).mean(), t_b.max(axis=1).mean(), 100.0 * (t_b.max(axis=1).mean() / t.max(axis=1).mean() - 1.0)))
    flags, order_b, tau_b, epoch_b = state()
    print("state at the end: flags %d, order %s, epoch %d" % (flags, order_b, epoch_b))
    plan.destroy()


if __name__ == "__main__":
    main()
