#!/usr/bin/env python3
"""Times audioSegmentation.music_thumbnailing_batch (kernels_simbatch.hpp, lib_similarity_batch.hpp) against the loop it replaces.
Writes profiles/bench_thumb_batch_n1_local.json.  Runs on the GPU.

Three workloads at 1.0 s / 0.5 s windows and thumb_size 10: 200 songs of 120 s at 8 kHz, 50 songs of 240 s at 16 kHz (eight
different synth_song clips taken in turn) and one song of 120 s alone.  Host to host, features included:
  batch     one call of music_thumbnailing_batch (times only: 48 bytes per clip come back),
  loop      music_thumbnailing clip after clip -- what a caller had before (it copies every filtered matrix back).
The two alternate for --repeats rounds after a warm-up; the median is reported beside every single time, and whether batch and
loop gave the same times.  Beside them the per-stage times of one batch run through the device entry points, the stream drained
between the stages (so their sum is above the call's own time), and the similarity stage's event time against the matrix work of
its Gram tiles (the stage is row statistics, normalisation and the Gram kernel: an upper bound for the kernel alone).  A record,
not a gate.

    python scripts/bench_thumb_batch.py [--repeats 5] [--short 200] [--long 50] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHORT_WINDOW, SHORT_STEP, THUMB = 1.0, 0.5, 10.0


def stage_split(clips, fs):
    """one batch through the device entry points with the stream drained between the stages: (ms per stage, similarity-stage
    event ms, Gram tiles, matrix flop)"""
    from pyaudioanalysis_amd import _ffi
    lib = _ffi.lib()
    window, step, m = int(fs * SHORT_WINDOW), int(fs * SHORT_STEP), int(round(THUMB / SHORT_STEP))
    n = len(clips)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in clips], out=offsets[1:])
    packed = np.concatenate(clips)
    ms = {}
    t0 = time.perf_counter()

    def mark(name):
        nonlocal t0
        _ffi.sync()
        t1 = time.perf_counter()
        ms[name] = (t1 - t0) * 1e3
        t0 = t1
    plan = _ffi.Plan(offsets, fs, window, step, deltas=True, sample_kind=0)
    d_in = _ffi.DeviceBuffer.from_host(packed)
    d_st = _ffi.DeviceBuffer(plan.out_doubles * 8)
    plan.execute(d_in, d_st)
    mark("features")
    feat_off = plan.out_offsets()
    n_vec = np.array([(len(c) - window) // step + 1 for c in clips], dtype=np.int64)
    R = n_vec - m + 1
    sim_off, filt_off = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    np.cumsum((n_vec * n_vec)[:-1], out=sim_off[1:])
    np.cumsum((R * R)[:-1], out=filt_off[1:])
    d_sim = _ffi.DeviceBuffer(int((n_vec * n_vec).sum()) * 8)
    d_filt = _ffi.DeviceBuffer(int((R * R).sum()) * 8)
    d_res = _ffi.DeviceBuffer(n * 48)
    mark("allocation")
    ev_ms = C.c_float()
    _ffi.check(lib.paa_timer_start())
    _ffi.check(lib.paa_dev_self_similarity_batch(d_st.ptr, plan.F, n, _ffi.as_i64p(feat_off), _ffi.as_i64p(n_vec), _ffi.as_i64p(n_vec),
                                                 d_sim.ptr, _ffi.as_i64p(sim_off)))
    _ffi.check(lib.paa_timer_stop(C.byref(ev_ms)))
    mark("similarity")
    _ffi.check(lib.paa_dev_thumbnail_filter_batch(d_sim.ptr, _ffi.as_i64p(sim_off), _ffi.as_i64p(n_vec), n, m, 5.0 / SHORT_STEP, 0.0, 1.0,
                                                  d_filt.ptr, _ffi.as_i64p(filt_off), d_res.ptr, C.c_void_p(d_res.ptr.value + n * 16)))
    mark("filter_fold_grow")
    d_res.to_host(np.int64, n * 6)
    mark("copy_back")
    for b in (d_in, d_st, d_sim, d_filt, d_res):
        b.free()
    plan.destroy()
    tiles = int(sum(t * (t + 1) // 2 for t in -(-n_vec // 128)))
    flop = tiles * 2.0 * 128 * 128 * plan.F
    return ms, float(ev_ms.value), tiles, flop


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short", type=int, default=200, help="songs of 120 s at 8 kHz")
    ap.add_argument("--long", type=int, default=50, help="songs of 240 s at 16 kHz")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_thumb_batch_n1_local.json"))
    args = ap.parse_args()
    from pyaudioanalysis_amd import _ffi, audioSegmentation as aS
    from synth import synth_song
    if _ffi.device_count() < 1:
        raise SystemExit("bench_thumb_batch.py needs a HIP device")
    _ffi.init(0)
    short = [synth_song(800 + k, 120.0, 8000) for k in range(8)]
    long_ = [synth_song(820 + k, 240.0, 16000) for k in range(8)]
    sets = {"200 x 120 s at 8 kHz": (8000, [short[i % 8] for i in range(args.short)]),
            "50 x 240 s at 16 kHz": (16000, [long_[i % 8] for i in range(args.long)]),
            "1 x 120 s at 8 kHz": (8000, short[:1])}
    out = {"short_window": SHORT_WINDOW, "short_step": SHORT_STEP, "thumb_size": THUMB, "repeats": args.repeats, "sets": {}}
    for name, (fs, clips) in sets.items():
        call = (fs, SHORT_WINDOW, SHORT_STEP, THUMB)
        fns = {"batch_host_s": lambda: aS.music_thumbnailing_batch(clips, *call),
               "loop_host_s": lambda: [aS.music_thumbnailing(c, *call)[:4] for c in clips]}
        rec = {"clips": len(clips), "seconds_per_clip": len(clips[0]) / fs, "sampling_rate": fs}
        times, last = {k: [] for k in fns}, {}
        for fn in fns.values():                         # warm-up: library, tables, plans, scratch
            fn()
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                last[k] = fn()
                times[k].append(time.perf_counter() - t0)
        for k, v in times.items():
            rec[k], rec[k + "_all"] = float(np.median(v)), v
        rec["loop_over_batch"] = rec["loop_host_s"] / rec["batch_host_s"]
        rec["batch_equals_loop"] = [tuple(r) for r in last["batch_host_s"]] == [tuple(r) for r in last["loop_host_s"]]
        stage_split(clips, fs)                          # warm-up of the split's own allocations
        ms, ev_ms, tiles, flop = stage_split(clips, fs)
        rec["stage_ms"] = ms
        rec["similarity_stage_event_ms"], rec["gram_tiles"], rec["gram_matrix_gflop"] = ev_ms, tiles, flop / 1e9
        rec["gram_matrix_tflops_over_stage"] = flop / (ev_ms * 1e-3) / 1e12 if ev_ms > 0 else None
        rec["vectors_per_clip"] = int((len(clips[0]) - int(fs * SHORT_WINDOW)) // int(fs * SHORT_STEP) + 1)
        print("%s: %s" % (name, json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")})), file=sys.stderr, flush=True)
        out["sets"][name] = rec
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: v[m] for m in ("batch_host_s", "loop_host_s", "loop_over_batch")} for k, v in out["sets"].items()}))


if __name__ == "__main__":
    main()
