#!/usr/bin/env python3
"""Times audioSegmentation.silence_removal_batch (kernels_onset.hpp, lib_onset.hpp) against the loop it replaces.  Writes
profiles/bench_silence_batch_n1_local.json.  Runs on the GPU.

Two data sets at 16 kHz with a 50 ms window and step: 200 clips of 20 s and 50 clips of 3 min (eight different synthetic clips
with digital silence between bursts, taken in turn; the long ones are nine of them in a row).  Host to host, features included:
  batch     one call of silence_removal_batch,
  loop      silence_removal(svm_fit="device") clip after clip -- what a caller had before,
  sklearn   silence_removal's default (scikit-learn trains the SVM) clip after clip, scikit-learn held to one thread.
The three alternate for --repeats rounds after a warm-up under one np.random.seed; the median is reported beside every single
time.  Beside them the per-stage times of one batch call (the stream is drained between the stages for it, so their sum is above
the call's own time) and whether batch and loop gave the same segments.  A record, not a gate; the scikit-learn figures are null
where it cannot be imported.

    python scripts/bench_silence_batch.py [--repeats 5] [--short 200] [--long 50] [--no-sklearn] [--out FILE]
"""
import argparse
import contextlib
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS = 16000
STAGES = ("features", "selection", "training_sets", "fits", "probability_threshold", "copy_back")


def base_clip(k):
    from synth import synth_clip
    x = synth_clip(700 + k, 20 * FS).copy()
    rng = np.random.default_rng(3 + k)
    for _ in range(8):                                  # digital silence between bursts
        a = int(rng.integers(0, 19 * FS))
        x[a:a + int(rng.integers(FS // 4, FS))] = 0
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short", type=int, default=200, help="clips of 20 s")
    ap.add_argument("--long", type=int, default=50, help="clips of 3 min")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_silence_batch_n1_local.json"))
    args = ap.parse_args()
    from pyaudioanalysis_amd import _ffi, audioSegmentation as aS
    if _ffi.device_count() < 1:
        raise SystemExit("bench_silence_batch.py needs a HIP device")
    _ffi.init(0)
    try:
        if args.no_sklearn:
            raise ImportError
        import sklearn.svm  # noqa: F401
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = None
    warnings.simplefilter("ignore")
    bases = [base_clip(k) for k in range(8)]
    sets = {"20 s": [bases[i % 8] for i in range(args.short)],
            "3 min": [np.concatenate([bases[(i + j) % 8] for j in range(9)]) for i in range(args.long)]}
    out = {"sampling_rate": FS, "st_win": 0.05, "st_step": 0.05, "repeats": args.repeats, "sets": {}}
    call = (FS, 0.05, 0.05)
    for name, clips in sets.items():
        fns = {"batch_host_s": lambda: aS.silence_removal_batch(clips, *call),
               "loop_device_fit_host_s": lambda: [aS.silence_removal(c, *call, svm_fit="device") for c in clips]}
        if threadpool_limits is not None:
            fns["loop_sklearn_host_s"] = lambda: [aS.silence_removal(c, *call) for c in clips]
        rec = {"clips": len(clips), "seconds_per_clip": len(clips[0]) / FS, "loop_sklearn_host_s": None}
        times, last = {k: [] for k in fns}, {}
        with (threadpool_limits(limits=1) if threadpool_limits is not None else contextlib.nullcontext()):
            for k, fn in fns.items():                   # warm-up: library, plans, scratch
                np.random.seed(5)
                fn()
            for _ in range(args.repeats):
                for k, fn in fns.items():
                    np.random.seed(5)
                    t0 = time.perf_counter()
                    last[k] = fn()
                    times[k].append(time.perf_counter() - t0)
        for k, v in times.items():
            rec[k], rec[k + "_all"] = float(np.median(v)), v
        rec["batch_over_loop_device_fit"] = rec["loop_device_fit_host_s"] / rec["batch_host_s"]
        if rec["loop_sklearn_host_s"] is not None:
            rec["batch_over_loop_sklearn"] = rec["loop_sklearn_host_s"] / rec["batch_host_s"]
        rec["batch_equals_loop_device_fit"] = last["batch_host_s"] == last["loop_device_fit_host_s"]
        stage_ms = np.zeros(6)
        np.random.seed(5)
        details = aS._silence_batch(clips, *call, 0.5, 0.5, lambda n: aS._batch_seeds(None, n), None, stage_ms=stage_ms)
        rec["stage_ms"] = dict(zip(STAGES, stage_ms.tolist()))
        rows = [len(d["alpha_y"]) for d in details]
        rec["frames_per_clip"], rec["svm_rows_min_max"] = len(details[0]["prob"]), [min(rows), max(rows)]
        rec["segments_total"] = int(sum(len(s) for s in last["batch_host_s"]))
        print("%s: %s" % (name, json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")})), file=sys.stderr, flush=True)
        out["sets"][name] = rec
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: v[m] for m in ("batch_host_s", "loop_device_fit_host_s", "loop_sklearn_host_s")} for k, v in out["sets"].items()}))


if __name__ == "__main__":
    main()
