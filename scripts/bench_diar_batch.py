#!/usr/bin/env python3
"""Times audioSegmentation.speaker_diarization_batch (kernels_diarbatch.hpp, lib_diar_batch.hpp) against the loop of
speaker_diarization_signal it replaces.  Writes profiles/bench_diar_batch_n1_local.json.  Runs on the GPU.

Workloads at 16 kHz with 1.0 s / 0.1 s mid-term windows, SVMs of the shipped shapes (seeded), planted speakers (four synthetic
voices that take turns every two seconds; eight different clips taken in turn): 200 clips of 120 s with n_speakers = 4 and again
with the sweep k = 2..9, 20 clips of 10 min with the sweep, one clip of an hour and one clip of 120 s alone, both with the sweep.
Host to host, features and SVMs included:
  batch     one call of speaker_diarization_batch,
  loop      speaker_diarization_signal clip after clip -- what a caller had before.
The two alternate for --repeats rounds after a warm-up; the median is reported beside every single time, and whether batch and
loop gave the same labels (a clip whose last k the HMM refuses counts as equal when both refuse it alike).  Beside them the
per-stage times of one batch run, the stream drained between the stages: features + SVMs, prepare, seeding, k-means with the
Lloyd rounds of the slowest job, silhouette inputs, copy-back of the labels, HMM.  A record, not a gate.

    python scripts/bench_diar_batch.py [--repeats 5] [--short 200] [--long 20] [--hour 3600] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS, MID_WINDOW, MID_STEP = 16000, 1.0, 0.1


def planted_clip(seed, seconds):
    """four synthetic voices in turns of two seconds, in an order drawn from `seed`"""
    from synth import synth_clip
    voices = [synth_clip(100 * seed + v, 2 * FS) for v in range(4)]
    order = np.random.default_rng(seed).integers(4, size=int(np.ceil(seconds / 2.0)))
    return np.concatenate([voices[v] for v in order])[:int(seconds * FS)]


def synthetic_models():
    """seeded SVMs of the shipped shapes (10 speakers, male / female) as load_model tuples"""
    import svc_libsvm
    from pyaudioanalysis_amd import audioTrainTest
    out = []
    for n_classes, seed in ((10, 1), (2, 2)):
        m = svc_libsvm.synthetic_model([4] * n_classes, 136, seed)
        clf = audioTrainTest.SvcArrays(m["support_vectors"], m["n_support"], m["dual_coef"], -m["rho"], m["prob_a"], m["prob_b"],
                                       m["gamma"], "rbf", np.arange(n_classes, dtype=np.float64))
        rng = np.random.default_rng(seed)
        out.append((clf, rng.standard_normal(136) * 0.1, 0.5 + rng.random(136), ["c%d" % i for i in range(n_classes)], 1.0, 0.1,
                    0.05, 0.05, False))
    return out


def outcome(fn):
    try:
        return fn()
    except (ValueError, IndexError) as exc:
        return exc


def same(a, b):
    if isinstance(a, BaseException) or isinstance(b, BaseException):
        return type(a) is type(b) and str(a) == str(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--short", type=int, default=200, help="clips of 120 s")
    ap.add_argument("--long", type=int, default=20, help="clips of 10 min")
    ap.add_argument("--hour", type=float, default=3600.0, help="seconds of the one long clip (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_diar_batch_n1_local.json"))
    args = ap.parse_args()
    from pyaudioanalysis_amd import _ffi, audioSegmentation as aS
    if _ffi.device_count() < 1:
        raise SystemExit("bench_diar_batch.py needs a HIP device")
    _ffi.init(0)
    models = synthetic_models()
    short = [planted_clip(k, 120.0) for k in range(8)]
    long_ = [planted_clip(20 + k, 600.0) for k in range(8)]
    sets = {}
    if args.short:
        sets["%d x 120 s, n_speakers = 4" % args.short] = ([short[i % 8] for i in range(args.short)], 4)
        sets["%d x 120 s, sweep" % args.short] = ([short[i % 8] for i in range(args.short)], 0)
    if args.long:
        sets["%d x 10 min, sweep" % args.long] = ([long_[i % 8] for i in range(args.long)], 0)
    if args.hour:
        sets["1 x %d s, sweep" % int(args.hour)] = ([planted_clip(40, args.hour)], 0)
    sets["1 x 120 s, sweep"] = (short[:1], 0)
    out = {"sampling_rate": FS, "mid_window": MID_WINDOW, "mid_step": MID_STEP, "repeats": args.repeats, "sets": {}}
    for name, (clips, n_speakers) in sets.items():
        kw = dict(models=models, random_state=3)
        fns = {"batch_host_s": lambda: aS.speaker_diarization_batch(clips, FS, n_speakers, MID_WINDOW, MID_STEP, on_error="record", **kw),
               "loop_host_s": lambda: [outcome(lambda: aS.speaker_diarization_signal(c, FS, n_speakers, MID_WINDOW, MID_STEP, **kw))
                                       for c in clips]}
        rec = {"clips": len(clips), "seconds_per_clip": len(clips[0]) / FS, "n_speakers": n_speakers}
        times, last = {k: [] for k in fns}, {}
        for fn in fns.values():                         # warm-up: library, tables, plans, models, scratch
            fn()
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                last[k] = fn()
                times[k].append(time.perf_counter() - t0)
        for k, v in times.items():
            rec[k], rec[k + "_all"] = float(np.median(v)), v
        rec["loop_over_batch"] = rec["loop_host_s"] / rec["batch_host_s"]
        rec["batch_equals_loop"] = all(same(a, b) for a, b in zip(last["batch_host_s"], last["loop_host_s"]))
        rec["clips_the_hmm_refuses"] = sum(isinstance(r, BaseException) for r in last["loop_host_s"])
        rec["windows_per_clip"] = int(len(last["loop_host_s"][0])) if not isinstance(last["loop_host_s"][0], BaseException) else None
        ms = {}
        aS._speaker_batch(aS._mono_clips(clips), FS, n_speakers, MID_WINDOW, MID_STEP, models, 3, None, False, "record", None, ms)
        rec["stage_ms"] = ms
        print("%s: %s" % (name, json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")})), file=sys.stderr, flush=True)
        out["sets"][name] = rec
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                  # after every set: a run that is cut short leaves what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({k: {m: v[m] for m in ("batch_host_s", "loop_host_s", "loop_over_batch", "batch_equals_loop")}
                      for k, v in out["sets"].items()}))


if __name__ == "__main__":
    main()
