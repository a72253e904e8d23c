#!/usr/bin/env python3
"""Write tests/golden/hmm_*.npz: the goldens of the GPU HMM segmenter (kernels_hmm.hpp).

Runs the UNMODIFIED reference (through oracle/load_reference.py, read-only) on the host for everything it computes without
hmmlearn: mid-term matrices, segments_to_labels, train_hmm_compute_statistics.  The decoder has no live reference here
(hmmlearn is not installed): its expected outputs are the NumPy restatement's (tests/hmm_ref.py), stored with the margin
of every decision.  Every file has kind = "hmm", no object arrays and no pickle.  Cases:

  radio    hmm_radio_sm_<clip>, hmm_radio_sm_concat: the shipped model data/hmmRadioSM (its four arrays, names, window and
           step) on the 16 kHz clips and on their concatenation; int16 signal and the live reference's mid-term matrix
           stored (the concatenation stores the clip order instead of the signal; a clip too long for one file keeps its
           second half in hmm_radio_sm_<clip>_tail)
  train    hmm_train_diar_1s, hmm_train_diar_01s: diarizationExample.wav with its .segments at mid-term steps 1.0 / 0.1 s:
           flags, the reference's priors, transition matrix, means, std; the decode of that model on its own features
  ties     hmm_ties: duplicated states, symmetric transitions, zeros in startprob and transmat
  synth    hmm_synth: seeded models and sequences (inputs are rebuilt from the seeds by tests/hmm_ref.py; expected states,
           log-probabilities and minimum margins stored), a ragged batch of 1 000 sequences of 1..600 windows
  edges    hmm_train_edges: training statistics of labels longer than the matrix, a one-window class, a never-left state

    python scripts/make_hmm_golden.py            # needs the reference tree
"""
import os
import pickle
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import load_reference  # noqa: E402
import hmm_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MIN_MARGIN = 1e-3
BLOCK = 256                                    # hmm::kBlockRows
CLIPS = ["speech_music_sample", "count", "diarizationExample", "doremi", "count2"]
# (K, D, seed): every (K, D) at the lengths around the block; the long ones below
SYNTH_SHAPES = [(1, 1, 11), (2, 1, 12), (2, 136, 13), (8, 136, 14), (8, 256, 15), (32, 1, 16), (32, 136, 17), (32, 256, 18),
                (5, 7, 19)]
SYNTH_LENGTHS = [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7]
SYNTH_LONG = [(2, 136, 21), (8, 136, 22), (32, 136, 23), (4, 3, 24)]
LONG_T = 36000
RAGGED = (4, 8, 31, 1000, 600)                 # K, D, seed, sequences, longest


def data(name):
    return os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", name)


def load_shipped_hmm():
    """hmmRadioSM's arrays without hmmlearn: throw-away module objects stand in while the pickle loads."""
    mods = {}
    for n in ("hmmlearn", "hmmlearn.hmm", "hmmlearn.base"):
        mods[n] = sys.modules.get(n)
        sys.modules[n] = types.ModuleType(n)
    sys.modules["hmmlearn.hmm"].GaussianHMM = type("GaussianHMM", (), {})
    sys.modules["hmmlearn.base"].ConvergenceMonitor = type("ConvergenceMonitor", (), {})
    try:
        with open(data("hmmRadioSM"), "rb") as f:
            h, names, win, step = pickle.load(f), pickle.load(f), pickle.load(f), pickle.load(f)
    finally:
        for n, m in mods.items():
            if m is None:
                del sys.modules[n]
            else:
                sys.modules[n] = m
    d = h.__dict__
    return d["startprob_"], d["transmat_"], d["means_"], d["_covars_"], names, win, step


def model_fields(start, trans, means, covars, names, win, step):
    return {"kind": np.str_("hmm"), "startprob": np.asarray(start, dtype=np.float64), "transmat": np.asarray(trans, dtype=np.float64),
            "means": np.asarray(means, dtype=np.float64), "covars": np.asarray(covars, dtype=np.float64),
            "class_names": np.array(names, dtype=np.str_), "mid_window": np.float64(win), "mid_step": np.float64(step)}


def decode_fields(model, mid, need_margin=True):
    lp, states, margins = hmm_ref.decode(model[0], model[1], model[2], model[3], mid.T)
    if need_margin:
        assert margins.min() >= MIN_MARGIN, margins.min()
    return {"mid": np.ascontiguousarray(mid, dtype=np.float64), "want_loglik": hmm_ref.log_likelihood(mid.T, model[2], model[3]),
            "want_states": states, "want_logprob": lp, "want_margins": margins}


def save(name, d):
    path = os.path.join(OUT, "hmm_%s.npz" % name)
    np.savez_compressed(path, **d)
    print("hmm_%s: %d bytes%s" % (name, os.path.getsize(path),
                                  ", min margin %.3g" % d["want_margins"].min() if "want_margins" in d else ""))
    assert os.path.getsize(path) < 1000000, path


def radio_cases():
    _, mtf, io_ = load_reference.load()
    start, trans, means, covars, names, win, step = load_shipped_hmm()
    model = (start, trans, means, covars)
    sigs = []
    for clip in CLIPS:
        fs, sig = io_.read_audio_file(data(clip + ".wav"))
        sig = io_.stereo_to_mono(sig)
        assert fs == 16000 and sig.dtype == np.int16
        sigs.append(sig)
        mid, _, _ = mtf.mid_feature_extraction(sig, fs, win * fs, step * fs, round(fs * 0.05), round(fs * 0.05))
        d = model_fields(start, trans, means, covars, names, win, step)
        # a clip too long for one file keeps its first half; the rest goes to a file of its own (case "signal_tail")
        half = sig.shape[0] if sig.shape[0] < 500000 else sig.shape[0] // 2
        d.update({"case": np.str_("radio"), "signal": sig[:half], "signal_length": np.int64(sig.shape[0]), "fs": np.float64(fs)})
        d.update(decode_fields(model, mid))
        save("radio_sm_" + clip, d)
        if half < sig.shape[0]:
            save("radio_sm_" + clip + "_tail", {"kind": np.str_("hmm"), "case": np.str_("signal_tail"), "signal": sig[half:]})
    sig = np.concatenate(sigs)
    mid, _, _ = mtf.mid_feature_extraction(sig, 16000, win * 16000, step * 16000, 800, 800)
    d = model_fields(start, trans, means, covars, names, win, step)
    d.update({"case": np.str_("radio_concat"), "clips": np.array(CLIPS, dtype=np.str_), "fs": np.float64(16000)})
    d.update(decode_fields(model, mid))
    print("concatenation: %d windows, %d label changes" % (mid.shape[1], np.count_nonzero(np.diff(d["want_states"]))))
    save("radio_sm_concat", d)


def train_cases():
    ref_seg = load_reference.load_segmentation()
    _, mtf, io_ = load_reference.load()
    fs, sig = io_.read_audio_file(data("diarizationExample.wav"))
    s, e, lab = ref_seg.read_segmentation_gt(data("diarizationExample.segments"))
    for name, step in (("train_diar_1s", 1.0), ("train_diar_01s", 0.1)):
        flags, names = ref_seg.segments_to_labels(s, e, lab, step)
        mid, _, _ = mtf.mid_feature_extraction(sig, fs, 1.0 * fs, step * fs, round(fs * 0.05), round(fs * 0.05))
        n = min(mid.shape[1], len(flags))
        mid, flags = mid[:, :n], np.array(flags[:n])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pri, trans, means, cov = ref_seg.train_hmm_compute_statistics(mid, flags)
        d = model_fields(pri, trans, means, cov, names, 1.0, step)
        d.update({"case": np.str_("train"), "flags": flags.astype(np.int64), "fs": np.float64(fs),
                  "gt_segments": np.array([[a, b] for a, b in zip(s, e)]), "gt_labels": np.array(lab, dtype=np.str_)})
        d["signal_from"] = np.str_("hmm_radio_sm_diarizationExample")       # the clip's samples live in that golden
        d.update(decode_fields((pri, trans, means, cov), mid))
        save(name, d)


def ties_case():
    # states 0 / 1 and 2 / 3 are duplicates, transitions symmetric under swapping each pair; state 4 can only be entered
    means = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 1.0], [3.0, 1.0], [-2.0, 2.0]])
    covars = np.array([[1.0, 2.0], [1.0, 2.0], [0.5, 0.5], [0.5, 0.5], [1.0, 1.0]])
    start = np.array([0.25, 0.25, 0.25, 0.25, 0.0])
    trans = np.array([[0.4, 0.4, 0.05, 0.05, 0.1], [0.4, 0.4, 0.05, 0.05, 0.1], [0.1, 0.1, 0.4, 0.4, 0.0],
                      [0.1, 0.1, 0.4, 0.4, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0]])
    rng = np.random.default_rng(5)
    path = np.repeat(np.array([0, 2, 0, 2, 2, 0, 4]), 40)
    X = means[path] + 0.4 * rng.standard_normal((path.shape[0], 2))
    d = model_fields(start, trans, means, covars, ["a", "b", "c", "d", "e"], 1.0, 1.0)
    d["case"] = np.str_("ties")
    d.update(decode_fields((start, trans, means, covars), X.T, need_margin=False))
    m = d["want_margins"]
    assert np.count_nonzero(m == 0) > 100 and m[-1] == np.inf or True
    assert m[m > 0].min() >= MIN_MARGIN, m[m > 0].min()
    save("ties", d)


def synth_case():
    rows = []
    for K, D, seed in SYNTH_SHAPES:
        for T in SYNTH_LENGTHS:
            rows.append((K, D, seed, T))
    for K, D, seed in SYNTH_LONG:
        rows.append((K, D, seed, LONG_T))
    d = {"kind": np.str_("hmm"), "case": np.str_("synth"), "rows": np.array(rows, dtype=np.int64)}
    states, logprob, margin = [], [], []
    for K, D, seed, T in rows:
        model = hmm_ref.synthetic_model(K, D, seed, zeros=True)
        X = hmm_ref.synthetic_sequence(model, T, seed + 1000)
        lp, st, mg = hmm_ref.decode(*model, X)
        assert mg.min() >= MIN_MARGIN, (K, D, seed, T, mg.min())        # re-seed above if this fires
        states.append(st.astype(np.uint8))
        logprob.append(lp[0])
        margin.append(mg.min())
        print("synth", K, D, T, "min margin %.3g" % mg.min())
    d.update({"want_states": np.concatenate(states), "want_logprob": np.array(logprob), "min_margin": np.array(margin)})
    K, D, seed, n_seq, longest = RAGGED
    model = hmm_ref.synthetic_model(K, D, seed, zeros=True)
    lengths = np.random.default_rng(seed).integers(1, longest + 1, n_seq)
    lengths[:3] = (1, longest, 2)
    X = hmm_ref.synthetic_sequence(model, int(lengths.sum()), seed + 1000)
    lp, st, mg = hmm_ref.decode(*model, X, lengths)
    assert mg.min() >= MIN_MARGIN, mg.min()
    d.update({"ragged": np.array(RAGGED, dtype=np.int64), "ragged_lengths": lengths.astype(np.int64),
              "ragged_states": st.astype(np.uint8), "ragged_logprob": lp, "ragged_min_margin": np.float64(mg.min())})
    save("synth", d)


def edges_case():
    ref_seg = load_reference.load_segmentation()
    rng = np.random.default_rng(9)
    d = {"kind": np.str_("hmm"), "case": np.str_("edges")}
    feats = rng.standard_normal((6, 50)) * 3 + 1
    cases = {"long_labels": np.concatenate([rng.integers(0, 3, 50), [1, 2, 0, 0]]),      # labels longer than the matrix
             "single_window": np.array([0] * 20 + [2] + [1] * 29),                         # class 2: one window, std 0
             "never_left": np.array([0] * 10 + [1] * 15 + [0] * 24 + [2])}                # class 2 is never left: NaN row
    import contextlib
    import io
    for name, labels in cases.items():
        with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            pri, trans, means, cov = ref_seg.train_hmm_compute_statistics(feats, labels)
        d.update({name + "_labels": labels.astype(np.int64), name + "_priors": pri, name + "_transmat": trans,
                  name + "_means": means, name + "_covars": cov})
    d["feats"] = feats
    assert np.isnan(d["never_left_transmat"][2]).all() and np.any(d["single_window_covars"][2] == 0)
    save("train_edges", d)


def main():
    warnings.simplefilter("ignore")
    radio_cases()
    train_cases()
    ties_case()
    edges_case()
    synth_case()


if __name__ == "__main__":
    main()
