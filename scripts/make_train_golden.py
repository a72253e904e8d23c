#!/usr/bin/env python3
"""Goldens of classifier tuning and training: what the UNMODIFIED reference's audioTrainTest.evaluate_classifier (:576-771) and
extract_features_and_train (:236-361) return, print and save on small seeded cases -> tests/golden/train_*.npz (data only).

Runs in the build container (the reference is imported through oracle/load_reference.py; no GPU).  Nothing of the reference is
edited: the splits, scalers and per-vector predictions are captured by WRAPPING the names evaluate_classifier looks up in its
module (train_test_split, group_split, StandardScaler, classifier_wrapper), the per-parameter confusion matrices by reading
its frame when it returns (sys.setprofile).  The train_test_split wrapper also checks, on every split, that the same global
state gives the same split over np.arange(n): a split IS two index lists.

    python scripts/make_train_golden.py            writes the four goldens (--only knn | sklearn | dir: one group)
    python scripts/make_train_golden.py --time     times the reference's kNN sweep on the bench shape (5 000 x 136, 88 splits)
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import load_reference  # noqa: E402
import knn_ref  # noqa: E402
import train_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEEDS = {"three": 101, "rare": 202, "sklearn": 303, "dir": 404}


def reference_module():
    load_reference.load_segmentation()
    return sys.modules["pyAudioAnalysis.audioTrainTest"]


class Recorder:
    """Wraps the names the reference's evaluate_classifier resolves in its own module."""

    def __init__(self, ref):
        self.ref, self.splits, self.scalers, self.preds, self.cms = ref, [], [], [], None
        self.saved = {n: getattr(ref, n) for n in ("train_test_split", "group_split", "StandardScaler", "classifier_wrapper")}

    def __enter__(self):
        rec, real = self, self.saved

        def train_test_split(X, y, test_size):
            state = np.random.get_state()
            out = real["train_test_split"](X, y, test_size=test_size)
            after = np.random.get_state()
            np.random.set_state(state)
            tr, te = real["train_test_split"](np.arange(len(X)), test_size=test_size)
            again = np.random.get_state()
            assert after[2] == again[2] and np.array_equal(after[1], again[1])
            assert np.array_equal(X[tr], out[0]) and np.array_equal(X[te], out[1]) and np.array_equal(y[te], out[3])
            rec.splits.append((tr, te))
            rec.preds.append([])
            return out

        def group_split(X, y, train_indeces, test_indeces, split_id):
            rec.splits.append((train_indeces[split_id], test_indeces[split_id]))
            rec.preds.append([])
            return real["group_split"](X, y, train_indeces, test_indeces, split_id)

        class StandardScaler(real["StandardScaler"]):
            def fit(self, X, y=None, **kw):
                out = super().fit(X, y, **kw)
                rec.scalers.append((self.mean_.copy(), self.scale_.copy()))
                return out

        def classifier_wrapper(classifier, classifier_type, test_sample):
            out = real["classifier_wrapper"](classifier, classifier_type, test_sample)
            rec.preds[-1].append(out[0])
            return out

        def profile(frame, event, arg):
            if event == "return" and frame.f_code is rec.ref.evaluate_classifier.__code__:
                rec.cms = np.array(frame.f_locals["cms_all"])

        for name, f in (("train_test_split", train_test_split), ("group_split", group_split), ("StandardScaler", StandardScaler),
                        ("classifier_wrapper", classifier_wrapper)):
            setattr(self.ref, name, f)
        sys.setprofile(profile)
        return self

    def __exit__(self, *exc):
        sys.setprofile(None)
        for name, f in self.saved.items():
            setattr(self.ref, name, f)


def record_run(ref, features, class_names, kind, params, mode, ids, n_exp, train_percentage, seed, splits=True):
    """One evaluate_classifier call of the reference as a dict of arrays."""
    np.random.seed(seed)
    text = io.StringIO()
    with Recorder(ref) as rec, contextlib.redirect_stdout(text):
        ret = ref.evaluate_classifier(features, class_names, kind, params, mode, ids, n_exp=n_exp, train_percentage=train_percentage)
    n_splits = len(rec.splits)
    assert n_splits == len(params) * n_exp and len(rec.scalers) == n_splits
    out = {"ret": np.array(ret), "text": np.array(text.getvalue()), "cms": rec.cms, "mode": np.array(mode), "n_exp": np.array(n_exp),
           "seed": np.array(seed), "train_percentage": np.array(train_percentage), "kind_name": np.array(kind),
           "has_ids": np.array(int(ids is not None)), "ids": np.array(ids if ids is not None else [], dtype=np.int64),
           "rng_after": np.random.get_state()[1].copy(), "rng_pos_after": np.array(np.random.get_state()[2])}
    if splits:
        out.update(train_off=np.concatenate([[0], np.cumsum([len(s[0]) for s in rec.splits])]).astype(np.int64),
                   test_off=np.concatenate([[0], np.cumsum([len(s[1]) for s in rec.splits])]).astype(np.int64),
                   train_idx=np.concatenate([s[0] for s in rec.splits]).astype(np.int32),
                   test_idx=np.concatenate([s[1] for s in rec.splits]).astype(np.int32),
                   mean=np.stack([s[0] for s in rec.scalers]), scale=np.stack([s[1] for s in rec.scalers]),
                   pred=np.concatenate([np.asarray(p, dtype=np.float64) for p in rec.preds]))
    return out


def save(name, common, runs):
    import sklearn
    out = dict(common, kind=np.array("train"), n_runs=np.array(len(runs)), sklearn_version=np.array(sklearn.__version__))
    for i, run in enumerate(runs):
        out.update({"r%d_%s" % (i, k): v for k, v in run.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d runs, %d bytes" % (name, len(runs), os.path.getsize(path)))
    return out


def common_of(features, class_names, params):
    return {"features": np.vstack(features), "class_sizes": np.array([len(f) for f in features]), "class_names": np.array(class_names),
            "params": np.array(params)}


def count_ambiguous(g):
    """kNN queries of a golden whose vote set the reference's unstable sort leaves undefined: must be none."""
    X, y = train_ref.features_to_matrix(train_ref.golden_features(g))
    n = total = 0
    for r in train_ref.golden_runs(g):
        for tr, te, mean, scale, k in train_ref.run_jobs(g, r):
            T, Q = (X[tr] - mean) / scale, (X[te] - mean) / scale
            n += int(knn_ref.ambiguous_vectors(T, y[tr], k, Q).sum())
            total += len(te)
    return n, total


def knn_goldens(ref):
    params = np.array(train_ref.KNN_PARAMS)
    feats, names = train_ref.three_class_features(), ["speech", "music", "noise"]
    g = save("train_knn_three", common_of(feats, names, params),
             [record_run(ref, feats, names, "knn", params, mode, None, 4, 0.9, SEEDS["three"]) for mode in (0, 1)])
    print("  ambiguous %d of %d" % count_ambiguous(g))
    assert count_ambiguous(g)[0] == 0
    feats, names = train_ref.rare_class_features(), ["a", "bb", "ccccc", "dddd"]
    params = np.array([1, 3, 5])
    ids = [i // 3 for i in range(sum(train_ref.RARE_SIZES))]
    g = save("train_knn_rare", common_of(feats, names, params),
             [record_run(ref, feats, names, "knn", params, mode, use_ids, 6, 0.8, SEEDS["rare"])
              for use_ids in (None, ids) for mode in (0, 1)])
    print("  ambiguous %d of %d" % count_ambiguous(g))
    assert count_ambiguous(g)[0] == 0


def sklearn_golden(ref):
    feats, names = train_ref.three_class_features(), ["speech", "music", "noise"]
    runs = []
    for kind, params in (("svm", [0.5, 5.0]), ("svm_rbf", [0.5, 5.0]), ("randomforest", [10, 25]), ("extratrees", [10, 25]),
                         ("gradientboosting", [10, 25])):
        run = record_run(ref, feats, names, kind, np.array(params), 1, None, 2, 0.9, SEEDS["sklearn"])
        run["params"] = np.array(params)
        runs.append(run)
    save("train_sklearn_small", common_of(feats, names, [0.0]), runs)


DIR_FS, DIR_SAMPLES, DIR_FILES = 8000, 2000, 75


def dir_signals():
    """Two class folders of 75 quarter-second clips each (tones against noise bursts).  MANY tiny files on purpose:
    extract_features_and_train calls evaluate_classifier with n_exp = -1, i.e. int(50000 / n_files) + 1 experiments per
    parameter value, and every experiment costs a split, a scaler and two sklearn.metrics calls on the host."""
    rng = np.random.default_rng(SEEDS["dir"])
    t = np.arange(DIR_SAMPLES) / float(DIR_FS)
    out = {}
    for i in range(DIR_FILES):
        f0, f1 = rng.uniform(200, 500), rng.uniform(900, 1500)
        tone = 6000 * np.sin(2 * np.pi * f0 * t) + 2500 * np.sin(2 * np.pi * f1 * t + rng.uniform(0, 6)) + 150 * rng.standard_normal(t.shape)
        out["tones/t%02d.wav" % i] = tone.astype(np.int16)
        envelope = np.exp(-((t - rng.uniform(0.05, 0.2)) / rng.uniform(0.02, 0.06)) ** 2)
        out["bursts/b%02d.wav" % i] = (rng.uniform(3000, 9000) * envelope * rng.standard_normal(t.shape) + 100 * rng.standard_normal(t.shape)).astype(np.int16)
    return out


def dir_golden(ref):
    import pickle
    import scipy.io.wavfile as wavfile
    signals = dir_signals()
    out = {"file_names": np.array(sorted(signals)), "fs": np.array(DIR_FS), "mid_window": np.array(1.0), "mid_step": np.array(0.5),
           "short_window": np.array(0.05), "short_step": np.array(0.05), "seed": np.array(SEEDS["dir"])}
    with tempfile.TemporaryDirectory() as d:
        for name, x in signals.items():
            os.makedirs(os.path.join(d, os.path.dirname(name)), exist_ok=True)
            wavfile.write(os.path.join(d, name), DIR_FS, x)
            out["wav_x_" + name] = x
        np.random.seed(SEEDS["dir"])
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            ref.extract_features_and_train([os.path.join(d, "tones"), os.path.join(d, "bursts")], 1.0, 0.5, 0.05, 0.05, "knn",
                                           os.path.join(d, "model_knn"))
        with open(os.path.join(d, "model_knn"), "rb") as fo:
            saved = [pickle.load(fo) for _ in range(11)]
    keys = ("features", "labels", "mean", "std", "class_names", "neighbors", "mid_window", "mid_step", "short_window", "short_step",
            "compute_beat")
    out.update({"saved_" + k: np.array(v) for k, v in zip(keys, saved)})
    out["selected_line"] = np.array([line for line in text.getvalue().splitlines() if line.startswith("Selected params")][0])
    save("train_dir_small", out, [])


def time_reference(ref, reps=1):
    """Wall time of the reference's evaluate_classifier("knn") on the bench shape of scripts/bench_classify.py --train."""
    feats = train_ref.bench_features()
    names = ["c%d" % c for c in range(len(feats))]
    np.random.seed(7)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        best = ref.evaluate_classifier(feats, names, "knn", np.array(train_ref.KNN_PARAMS), 1, None, n_exp=-1, train_percentage=0.9)
    dt = time.perf_counter() - t0
    rec = {"what": "the unmodified reference's evaluate_classifier('knn') on the build container's CPU (scripts/make_train_golden.py --time)",
           "samples": int(sum(len(f) for f in feats)), "dims": int(feats[0].shape[1]), "classes": len(feats), "params": train_ref.KNN_PARAMS,
           "n_exp": int(50000 / sum(len(f) for f in feats)) + 1, "train_percentage": 0.9, "best_param": int(best), "seconds": dt,
           "cpus": os.cpu_count()}
    path = os.path.join(ROOT, "profiles", "bench_train_reference_cpu.json")
    json.dump(rec, open(path, "w"), indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--only", choices=("knn", "sklearn", "dir"), help="write the goldens of this group only")
    args = ap.parse_args()
    ref = reference_module()
    if args.time:
        return time_reference(ref)
    for group, make in (("knn", knn_goldens), ("sklearn", sklearn_golden), ("dir", dir_golden)):
        if args.only in (None, group):
            make(ref)


if __name__ == "__main__":
    main()
