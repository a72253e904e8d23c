"""NumPy restatement of pyAudioAnalysis's classifier tuning (audioTrainTest.evaluate_classifier, :576-771) over index-list
jobs -- the CPU second opinion for pyaudioanalysis_amd.audioTrainTest.evaluate_classifier and for the kNN split-sweep kernel
(pyaudioanalysis_amd/csrc/kernels_knn.hpp, knn_split_kernel).  Test helper, not part of the package.

A split is two index lists over the stacked sample matrix plus the mean / scale of its training rows; what is fitted on a
split and how a test row is classified are the caller's (`fit`, `classify`): knn_ref.classify for kNN, scikit-learn's
per-vector predict for the rest.  The confusion matrix and the macro F1 of a split are written out in NumPy (for what
evaluate_classifier prints they agree with sklearn.metrics), so the kNN checks need no scikit-learn."""
import io
import os

import numpy as np

import knn_ref

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

THREE_SIZES, THREE_DIMS = (60, 45, 30), 20
RARE_SIZES, RARE_DIMS = (25, 2, 18, 2), 9
KNN_PARAMS = [1, 3, 5, 7, 9, 11, 13, 15]


# ---------------------------------------------------------------------------------------------------------------------
# seeded generators
# ---------------------------------------------------------------------------------------------------------------------
def class_features(sizes, n_dims, seed, spread=1.6):
    """One [n][n_dims] matrix per class: Gaussian blobs close enough to be confused, on features of unequal scale."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((len(sizes), n_dims))
    widths = rng.uniform(0.5, 3.0, n_dims)
    return [(centres[c] + spread * rng.standard_normal((n, n_dims))) * widths + 10.0 * c / len(sizes) for c, n in enumerate(sizes)]


def three_class_features(seed=11):
    return class_features(THREE_SIZES, THREE_DIMS, seed)


def rare_class_features(seed=12):
    return class_features(RARE_SIZES, RARE_DIMS, seed)


def bench_features(n_samples=5000, n_dims=136, n_classes=8, seed=5):
    """The measured shape of scripts/bench_classify.py --train: equal classes."""
    return class_features([n_samples // n_classes] * n_classes, n_dims, seed, spread=2.5)


def features_to_matrix(features):
    X = np.vstack(features)
    y = np.concatenate([c * np.ones(len(f)) for c, f in enumerate(features)])
    return X, y


def seeded_jobs(n_samples, n_dims, n_jobs, seed, k_max=32):
    """(X, labels, jobs) of random Gaussian samples and random index-list jobs (lists permuted, overlapping between jobs),
    each with the mean / population deviation of its training rows."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_samples, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    labels = rng.integers(0, 5, n_samples).astype(np.float64)
    jobs = []
    for _ in range(n_jobs):
        perm = rng.permutation(n_samples)
        n_train = int(rng.integers(n_samples // 2, n_samples - 3))
        tr, te = perm[:n_train], perm[n_train:]
        jobs.append((tr, te, X[tr].mean(axis=0), X[tr].std(axis=0), int(rng.integers(1, k_max + 1))))
    return X, labels, jobs


# ---------------------------------------------------------------------------------------------------------------------
# goldens
# ---------------------------------------------------------------------------------------------------------------------
def load_golden(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_features(g):
    """The list of per-class matrices a golden's stacked features came from."""
    ends = np.cumsum(g["class_sizes"])
    return [g["features"][e - n:e] for e, n in zip(ends, g["class_sizes"])]


def golden_runs(g):
    """The run prefixes of a golden ("r0_", "r1_", ...)."""
    return ["r%d_" % i for i in range(int(g["n_runs"]))]


def run_splits(g, r):
    """[(train_idx, test_idx, mean, scale)] of run r, one per (parameter, experiment), parameter-major."""
    tro, teo = g[r + "train_off"], g[r + "test_off"]
    return [(g[r + "train_idx"][tro[s]:tro[s + 1]], g[r + "test_idx"][teo[s]:teo[s + 1]], g[r + "mean"][s], g[r + "scale"][s])
            for s in range(len(tro) - 1)]


def run_jobs(g, r):
    """The kNN jobs (train_idx, test_idx, mean, scale, k) of run r."""
    n_exp = int(g[r + "n_exp"])
    return [(tr, te, mean, scale, int(g["params"][s // n_exp])) for s, (tr, te, mean, scale) in enumerate(run_splits(g, r))]


def run_ids(g, r):
    return g[r + "ids"].tolist() if int(g[r + "has_ids"]) else None


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def confusion_matrix(y_true, y_pred):
    """Counts [true][predicted] over the sorted union of the labels that occur (sklearn.metrics.confusion_matrix)."""
    y_true, y_pred = np.asarray(y_true, dtype=np.float64), np.asarray(y_pred, dtype=np.float64)
    classes = np.unique(np.concatenate([y_true, y_pred]))
    cm = np.zeros((classes.shape[0], classes.shape[0]), dtype=np.int64)
    for t, p in zip(np.searchsorted(classes, y_true), np.searchsorted(classes, y_pred)):
        cm[t, p] += 1
    return cm


def macro_f1(y_true, y_pred):
    """Mean over the occurring labels of 2 tp / (2 tp + fp + fn), 0 where that is 0 / 0 (sklearn.metrics.f1_score, macro)."""
    cm = confusion_matrix(y_true, y_pred)
    tp = np.diagonal(cm).astype(np.float64)
    denom = cm.sum(axis=0) + cm.sum(axis=1)
    return float(np.mean(np.where(denom > 0, 2 * tp / np.maximum(denom, 1), 0.0)))


def knn_fit(Xs, y, k):
    return Xs, y, int(k)


def knn_classify(model, Xs):
    return [np.int64(v) for v in knn_ref.classify(model[0], model[1], model[2], Xs)[0]]


def sklearn_fit(kind):
    def fit(Xs, y, param):
        import sklearn.ensemble
        import sklearn.svm
        if kind in ("svm", "svm_rbf"):
            m = sklearn.svm.SVC(C=param, kernel="rbf" if kind == "svm_rbf" else "linear", probability=True, gamma="auto")
        else:
            m = {"randomforest": sklearn.ensemble.RandomForestClassifier, "extratrees": sklearn.ensemble.ExtraTreesClassifier,
                 "gradientboosting": sklearn.ensemble.GradientBoostingClassifier}[kind](n_estimators=param)
        return m.fit(Xs, y)
    return fit


def sklearn_classify(model, Xs):
    return [model.predict(x.reshape(1, -1))[0] for x in Xs]


def random_split_source(n_samples, train_percentage):
    """next_split of evaluate(): a random split per call from NumPy's global state (scikit-learn's train_test_split over
    the indices) with scikit-learn's scaler of its training rows."""
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import StandardScaler

    def next_split(X, p, e):
        tr, te = train_test_split(np.arange(n_samples), test_size=1 - train_percentage)
        sc = StandardScaler().fit(X[tr])
        return tr, te, sc.mean_, sc.scale_
    return next_split


def listed_split_source(splits, n_exp):
    return lambda X, p, e: splits[p * n_exp + e]


def confusion_text(cm, class_names):
    short = [c[0:3] if len(c) > 4 else c for c in class_names]
    text = "".join("\t%s" % c for c in short) + "\n"
    for i, c in enumerate(short):
        text += c + "".join("\t{0:.2f}".format(100.0 * cm[i][j] / np.sum(cm)) for j in range(len(short))) + "\n"
    return text


def evaluate(features, class_names, params, parameter_mode, n_exp, next_split, fit, classify):
    """(chosen parameter, confusion matrix per parameter, predictions per split, printed text).  next_split(X, p, e) gives
    split e of parameter p as (train_idx, test_idx, mean, scale) and is called parameter-major, each call followed by that
    split's fit -- the order in which the reference consumes NumPy's global state."""
    X, y = features_to_matrix(features)
    n_classes = len(features)
    out = io.StringIO()
    cms, preds, acc, f1s, f1_std, pres, recs, f1c = [], [], [], [], [], [], [], []
    for p, param in enumerate(params):
        cm = np.zeros((n_classes, n_classes))
        f1_exp = []
        for e in range(n_exp):
            out.write("Param = {0:.5f} - classifier Evaluation Experiment {1:d} of {2:d}\n".format(param, e + 1, n_exp))
            tr, te, mean, scale = next_split(X, p, e)
            model = fit((X[tr] - mean) / scale, y[tr], param)
            y_pred = classify(model, (X[te] - mean) / scale)
            preds.append(np.array(y_pred, dtype=np.float64))
            cmt = confusion_matrix(y[te], y_pred)
            f1_exp.append(macro_f1(y[te], y_pred))
            if cmt.size != cm.size:
                present = set(np.asarray(y[te]).tolist()) | set(float(v) for v in y_pred)
                missing = [int(c) for c in sorted(set(y.tolist()) - present)]
                for c in missing:
                    cmt = np.insert(cmt, c, 0, axis=0)
                for c in missing:
                    cmt = np.insert(cmt, c, 0, axis=1)
            cm = cm + cmt
        cm = cm + 0.0000000010
        rec = np.array([cm[c, c] / np.sum(cm[c, :]) for c in range(n_classes)])
        pre = np.array([cm[c, c] / np.sum(cm[:, c]) for c in range(n_classes)])
        f1 = 2 * rec * pre / (rec + pre)
        cms.append(cm)
        pres.append(pre)
        recs.append(rec)
        f1c.append(f1)
        acc.append(np.sum(np.diagonal(cm)) / np.sum(cm))
        f1s.append(np.mean(f1))
        f1_std.append(np.std(f1_exp))
    out.write("\t\t" + "".join("%s\t\t" % c if i == len(class_names) - 1 else "%s\t\t\t" % c for i, c in enumerate(class_names)))
    out.write("OVERALL\n\tC" + "\tPRE\tREC\tf1" * len(class_names) + "\tACC\tf1\n")
    best_acc, best_f1 = int(np.argmax(acc)), int(np.argmax(f1s))
    for i in range(len(params)):
        out.write("\t{0:.3f}".format(params[i]))
        for c in range(n_classes):
            out.write("\t{0:.1f}\t{1:.1f}\t{2:.1f}".format(100.0 * pres[i][c], 100.0 * recs[i][c], 100.0 * f1c[i][c]))
        out.write("\t{0:.1f}\t{1:.1f}".format(100.0 * acc[i], 100.0 * f1s[i]))
        out.write(("\t best f1" if i == best_f1 else "") + ("\t best Acc" if i == best_acc else "") + "\n")
    best = best_acc if parameter_mode == 0 else best_f1
    out.write("Confusion Matrix:\n" + confusion_text(cms[best], class_names))
    if parameter_mode == 1:
        out.write("Best macro f1 {0:.1f}\n".format(100 * f1s[best]))
        out.write("Best macro f1 std {0:.1f}\n".format(100 * f1_std[best]))
    return params[best], np.array(cms), preds, out.getvalue()
