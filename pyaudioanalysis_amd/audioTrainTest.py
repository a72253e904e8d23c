"""Drop-in for the classification and regression halves of pyAudioAnalysis.audioTrainTest (reference:
pyAudioAnalysis/audioTrainTest.py).

    load_model(model_name, is_regression=False)                  audioTrainTest.py:523-553
    classifier_wrapper(classifier, classifier_type, test_sample) audioTrainTest.py:52-94
    file_classification(input_file, model_name, model_type)      audioTrainTest.py:1052-1096
    file_classification_batch(files, model_name, model_type)     many files: one mid-term plan, one classifier launch
    Knn(features, labels, neighbors), load_model_knn(name)       audioTrainTest.py:33-49, :492-520
    forest_model(classifier), forest_predict(...), ForestArrays   the tree ensembles of classifier_wrapper (:84-93)
    regression_wrapper(model, model_type, test_sample)            audioTrainTest.py:96-111
    train_svm_regression, train_random_forest_regression          audioTrainTest.py:222-233
    feature_extraction_train_regression(...)                      audioTrainTest.py:370-489
    evaluate_regression(features, labels, n_exp, method, params)  audioTrainTest.py:774-855
    file_regression(input_file, model_name, model_type)           audioTrainTest.py:1099-1151
    file_regression_batch(files, model_name, model_type)          many files: one mid-term plan, one regression launch
    regress(models, model_type, feats, means, stds), SvrBank, SvrArrays   every model on every vector in one launch
    train_knn, train_svm, train_random_forest, train_gradient_boosting, train_extra_trees   audioTrainTest.py:117-219
    features_to_matrix, group_split, print_confusion_matrix       audioTrainTest.py:887-911, :556-573, :858-884
    evaluate_classifier(features, class_names, classifier_name, params, parameter_mode, ...)   audioTrainTest.py:576-771
    extract_features_and_train(paths, ..., classifier_type, model_name, ...)                   audioTrainTest.py:236-361
    knn_split_predict(X, labels, jobs, proba=False, neighbors=False)   every kNN split of a sweep in one launch
    svm_split_fit_predict(X, labels, jobs, kernel, ..., kernel_cache="none"), smo_solve(X, tasks, ...)   every SVM fit of a sweep side by side on the GPU
    smo_cache_layout(task_rows, groups, cache_bytes)              the layout of kernel_cache="gram": one resident kernel matrix per group of tasks
    train_svm_device(features, labels, c_param, kernel, random_state=None), to_sklearn_svc(model)   SVC(probability=True).fit on the GPU
    svc_fit_proba(X, labels, jobs, kernel, ...), platt_sigmoid(dec, signs, offsets)   its stages: fits, folds and sigmoids; the sigmoid alone
    svr_split_fit_predict(X, y, jobs, kernel, ..., kernel_cache="none"), svr_solve(X, y, tasks, ...)   every SVR fit of a sweep side by side on the GPU
    train_svm_regression_device(features, labels, c_param, kernel), to_sklearn_svr(model), svr_kernel_matrix(X, tasks, kernel)   SVR.fit on the GPU
    forest_split_fit_predict(X, labels, jobs, kind, proba=False), tree_fit(X, tasks, splitter)   every forest fit of a sweep side by side on the GPU
    train_forest_device(features, labels, n_estimators, kind, random_state=None), to_sklearn_forest(arrays, kind)   the forests' fit on the GPU

For the model types "svm" / "svm_rbf" (the shipped SVC(probability=True) models of data/models) predict() and
predict_proba() run on the GPU (kernels_svc.hpp through paa_svc_*): libsvm's decision values, votes, Platt sigmoids and
pairwise coupling for every vector in one launch.  Only the fitted model's arrays are read (support_vectors_,
n_support_, _dual_coef_, _intercept_, probA_, probB_, _gamma, kernel, classes_), so a model given as those arrays
(SvcArrays) works without scikit-learn.  For "knn" (the shipped knn_* models: pickled NumPy arrays, no scikit-learn)
Knn.classify runs on the GPU (kernels_knn.hpp through paa_knn_*): distances to every training row, the k nearest in
ascending (squared distance, training index) and the votes, for every vector in one launch.  For "randomforest",
"extratrees" and "gradientboosting" (scikit-learn's RandomForestClassifier, ExtraTreesClassifier and
GradientBoostingClassifier, as the reference's trainers make them) predict() and predict_proba() run on the GPU
(kernels_forest.hpp through paa_forest_*): every tree walked for every vector, the leaf values summed in tree order,
bit-identical to scikit-learn; only the trees' tree_ arrays, classes_ and (boosted) learning_rate / init_ are read, so a
model given as arrays (ForestArrays) works without scikit-learn.  Unpickling an SVM or tree-ensemble model needs
scikit-learn exactly where the reference needs it (load_model).  Training stays with scikit-learn: evaluate_classifier / extract_features_and_train tune and train all six
types; for "knn", which has no fit, the whole split sweep of evaluate_classifier is ONE launch over index lists into one
resident sample matrix (knn_split_kernel through paa_knn_splits_f64); the five scikit-learn types gain only the removal of
the per-vector predict loop -- by default.  With svm_fit="device" evaluate_classifier fits "svm" / "svm_rbf" on the GPU too:
every pair of classes of every split is a binary C-SVC problem of smo_kernel (libsvm's solver without shrinking, FP64; no Platt
cross-validation, whose probabilities the sweep never reads), all of them side by side (paa_svc_fit_splits_f64); the final
fit of extract_features_and_train and its model file are scikit-learn's by default.  train_svm_device is train_svm on the GPU,
Platt probabilities included (paa_svc_fit_proba_f64: per pair the full fit and libsvm's five cross-validation fits for
scikit-learn's seed as smo_kernel tasks, the held-out rows scored by svc_pairs_kernel, probA_ / probB_ by platt_sigmoid_kernel);
to_sklearn_svc makes a real SVC of its result, which extract_features_and_train(final_fit="device") pickles as the model file.
With forest_fit="device" "randomforest" / "extratrees" are fitted on the GPU too: one workgroup per tree builds scikit-learn's
depth-first Gini tree bit for bit (tree_fit_kernel through paa_tree_fit_tasks_f64 / paa_forest_fit_splits_f64; the host draws the
tree seeds, rand_r seeds and bootstrap counts NumPy draws for scikit-learn), the sweep scores every test row with the predict
kernels, train_forest_device is the final fit and to_sklearn_forest makes the model file's RandomForestClassifier /
ExtraTreesClassifier.
With boosting_fit="device" "gradientboosting" is fitted on the GPU as well: per stage one launch forms the negative gradients and the
loss of the stage before (boost_gradient_kernel) and one builds the stage's depth-3 Friedman trees, one workgroup per (split, class),
with the leaves' Newton steps (paa_boost_fit_splits_f64; boosting_split_fit_predict, train_gradient_boosting_device,
to_sklearn_boosting, tree_fit_boosting).
smote / use_smote are refused (NotImplementedError).
Regression ("svm" / "svm_rbf": sklearn.svm.SVR; "randomforest": RandomForestRegressor) predicts on the GPU too: a BANK of
SVR models -- file_regression's model_name_* models, each with its own MEANS file, or the n_exp models of one parameter
value of evaluate_regression -- scores every vector in one launch (kernels_svr.hpp through paa_svr_*: libsvm's decision value
in the model's support-vector order, each model after its own standardisation); a forest regressor is the averaged forest
with one output (paa_forest_create kind 2), bit-identical to RandomForestRegressor.predict.  Only the fitted arrays are read
(SVR: support_vectors_, _dual_coef_, _intercept_, _gamma, kernel), so SvrArrays / ForestArrays(kind="regressor") work
without scikit-learn; the fits of the trainers and of evaluate_regression are scikit-learn's and dominate their run time --
by default.  With svm_fit="device" evaluate_regression fits "svm" / "svm_rbf" on the GPU too: every split of every parameter
value is one epsilon-SVR problem of svr_smo_kernel (libsvm's solver without shrinking, FP64; a dual of 2 n variables over n
rows whose kernel rows are formed once per row), all of them side by side, scored in the same call
(paa_svr_fit_splits_f64); kernel_cache="gram" solves from resident kernel matrices with the same bytes out, and
final_fit="device" makes the final fit of feature_extraction_train_regression and its model file the device's too.
With forest_fit="device" evaluate_regression fits "randomforest" on the GPU: one workgroup per tree builds scikit-learn's
squared-error regression tree (the MSE instance of tree_fit_kernel through paa_tree_fit_reg_tasks_f64 /
paa_forest_reg_fit_splits_f64), every floating-point sum in a fixed order -- scikit-learn's bits when the targets make the sums
exact, a valid CART tree otherwise (tree_fit_regression); train_random_forest_regression_device is the final fit and
to_sklearn_forest_regressor makes the model file's RandomForestRegressor.
"""
import collections
import ctypes as C
import os
import pickle as cPickle
import weakref

import numpy as np

from . import MidTermFeatures as aF
from . import _ffi, audioBasicIO

_SVM_TYPES = ("svm", "svm_rbf")
_FOREST_TYPES = ("randomforest", "extratrees", "gradientboosting")
_KERNEL_TYPES = {"linear": 0, "rbf": 2}          # libsvm's LINEAR / RBF
_FOREST_KINDS = {"averaged": 0, "boosted": 1, "regressor": 2}      # PAA_FOREST_AVERAGED / _BOOSTED / _REGRESSOR
_REGRESSION_TYPES = ("svm", "svm_rbf", "randomforest")


class SvcArrays:
    """A fitted multi-class probabilistic SVC given by its arrays in scikit-learn's attribute names (e.g. from an .npz);
    dual_coef / intercept are the PRIVATE _dual_coef_ / _intercept_ (libsvm's sv_coef and -rho)."""

    def __init__(self, support_vectors, n_support, dual_coef, intercept, prob_a, prob_b, gamma, kernel, classes):
        self.support_vectors_ = np.asarray(support_vectors, dtype=np.float64)
        self.n_support_ = np.asarray(n_support, dtype=np.int32)
        self._dual_coef_ = np.asarray(dual_coef, dtype=np.float64)
        self._intercept_ = np.asarray(intercept, dtype=np.float64)
        self.probA_ = np.asarray(prob_a, dtype=np.float64)
        self.probB_ = np.asarray(prob_b, dtype=np.float64)
        self._gamma = float(gamma)
        self.kernel = str(kernel)
        self.classes_ = np.asarray(classes)


def _stats(mean, std, n_dims):
    mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(-1))
    std = np.ascontiguousarray(np.asarray(std, dtype=np.float64).reshape(-1))
    if mean.shape[0] != n_dims or std.shape[0] != n_dims:
        raise ValueError("mean / std of %d / %d values for a model of %d dims" % (mean.shape[0], std.shape[0], n_dims))
    return mean, std


def _class_indices(raw, bound=2**31):
    """Raw labels [n] as int32 class indices: an integer-valued label in 0 .. bound - 1 is its own index, every other label
    (fractional, negative, too large, no number) is -1 and counts for no class."""
    labels = np.full(raw.shape[0], -1, dtype=np.int32)
    if raw.dtype.kind in "biuf":
        v = raw.astype(np.float64)
        ok = (v == np.floor(v)) & (v >= 0) & (v < bound)
        labels[ok] = v[ok].astype(np.int32)
    return labels


class _DeviceModel:
    """A model uploaded to the device once and freed with the object.  A subclass sets n_dims, n_classes and the handle
    (_adopt) and names what differs: _family ("svc": paa_svc_predict_f64, paa_svc_dev_predict_f64, paa_svc_destroy),
    _index_dtype of the indices it returns, _extra (attribute holding the row width, dtype, pointer type) of the optional
    third output of its entry points, classes (None: callers get the class index itself) and _raise_invalid for the raw indices of a call."""
    _index_dtype = np.int64
    _extra = None
    classes = None

    def _adopt(self, handle):
        self.handle = handle
        self._finalizer = weakref.finalize(self, getattr(_ffi.lib(), "paa_%s_destroy" % self._family), handle)

    def _raise_invalid(self, idx):
        pass

    def labels(self, idx):
        """What the reference's classifier_wrapper returns for these indices: classes_ of an SVM or tree ensemble, a kNN's
        class index."""
        return idx if self.classes is None else self.classes[idx]

    def predict(self, feats, mean, std, extra=False):
        """feats [n_dims][n_vec] (feature-major) -> (indices [n_vec], probabilities [n_vec][n_classes]) of
        (feats[:, v] - mean) / std, plus the third output [n_vec][width] when extra is true."""
        F = np.ascontiguousarray(feats, dtype=np.float64)
        if F.ndim != 2 or F.shape[0] != self.n_dims or F.shape[1] < 1:
            raise ValueError("feature matrix of shape %s for a model of %d dims" % (F.shape, self.n_dims))
        mean, std = _stats(mean, std, self.n_dims)
        n = F.shape[1]
        idx = np.empty(n, dtype=np.int32)
        proba = np.empty((n, self.n_classes), dtype=np.float64)
        third = np.empty((n, getattr(self, self._extra[0])), dtype=self._extra[1]) if extra else None
        tail = () if self._extra is None else (third.ctypes.data_as(self._extra[2]) if extra else None,)
        _ffi.check(getattr(_ffi.lib(), "paa_%s_predict_f64" % self._family)(
            self.handle, _ffi.as_f64p(F), self.n_dims, n, n, _ffi.as_f64p(mean), _ffi.as_f64p(std),
            idx.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(proba), *tail))
        self._raise_invalid(idx)
        idx = idx.astype(self._index_dtype, copy=False)
        return (idx, proba, third) if extra else (idx, proba)

    def predict_device(self, d_feats, ld, n_vec, mean, std):
        """The same on a device-resident matrix (a DeviceBuffer holding [n_dims][ld] doubles)."""
        mean, std = _stats(mean, std, self.n_dims)
        bufs = []
        try:
            bufs.append(_ffi.DeviceBuffer.from_host(np.concatenate([mean, std])))
            bufs.append(_ffi.DeviceBuffer(max(4 * n_vec, 8)))
            bufs.append(_ffi.DeviceBuffer(8 * n_vec * self.n_classes))
            d_stats, d_idx, d_proba = bufs
            _ffi.check(getattr(_ffi.lib(), "paa_%s_dev_predict_f64" % self._family)(
                self.handle, d_feats.ptr, self.n_dims, ld, n_vec, d_stats.ptr, C.c_void_p(d_stats.ptr.value + 8 * self.n_dims),
                d_idx.ptr, d_proba.ptr, *(() if self._extra is None else (None,))))
            idx = d_idx.to_host(np.int32, n_vec)
            proba = d_proba.to_host(np.float64, n_vec * self.n_classes).reshape(n_vec, self.n_classes)
        finally:
            for b in bufs:
                b.free()
        self._raise_invalid(idx)
        return idx.astype(self._index_dtype, copy=False), proba


_uploaded = {}          # model class -> WeakKeyDictionary: classifier -> its device model


def _device_model(cls, classifier, make=None, still_valid=None):
    """The device copy of a classifier (uploaded at the first use, kept while the classifier lives; an object that cannot
    be weakly referenced or hashed is uploaded at every call).  make(classifier) builds it where cls(classifier) does
    not; a kept copy for which still_valid(copy) is false is replaced."""
    if isinstance(classifier, cls):
        return classifier
    cache = _uploaded.setdefault(cls, weakref.WeakKeyDictionary())
    try:
        m = cache.get(classifier)
    except TypeError:
        m = None
    if m is None or (still_valid is not None and not still_valid(m)):
        m = (make or cls)(classifier)
        try:
            cache[classifier] = m
        except TypeError:
            pass
    return m


class SvcModel(_DeviceModel):
    """A fitted SVC on the device (paa_svc_create)."""
    _family = "svc"
    _index_dtype = np.int32

    def __init__(self, classifier):
        kernel = str(getattr(classifier, "kernel", ""))
        if kernel not in _KERNEL_TYPES:
            raise NotImplementedError("SVC kernel %r: the GPU path serves 'rbf' and 'linear' models" % (kernel,))
        sv = np.ascontiguousarray(classifier.support_vectors_, dtype=np.float64)
        n_support = np.ascontiguousarray(classifier.n_support_, dtype=np.int32)
        coef = np.ascontiguousarray(classifier._dual_coef_, dtype=np.float64)
        rho = np.ascontiguousarray(-np.asarray(classifier._intercept_, dtype=np.float64).reshape(-1))
        prob_a = np.ascontiguousarray(np.asarray(classifier.probA_, dtype=np.float64).reshape(-1))
        prob_b = np.ascontiguousarray(np.asarray(classifier.probB_, dtype=np.float64).reshape(-1))
        k = n_support.shape[0]
        pairs = k * (k - 1) // 2
        if sv.ndim != 2 or coef.shape != (k - 1, sv.shape[0]) or rho.shape[0] != pairs or prob_a.shape[0] != pairs \
                or prob_b.shape[0] != pairs:
            raise ValueError("not a fitted probabilistic SVC (SVC(probability=True)): inconsistent arrays")
        self.classes = np.asarray(classifier.classes_)
        self.n_classes = k
        self.n_dims = sv.shape[1]
        gamma = float(classifier._gamma) if kernel == "rbf" else 0.0
        handle = C.c_void_p()
        _ffi.check(_ffi.lib().paa_svc_create(_ffi.as_f64p(sv), sv.shape[0], sv.shape[1], n_support.ctypes.data_as(_ffi.c_i32p), k,
                                             _ffi.as_f64p(coef), _ffi.as_f64p(rho), _ffi.as_f64p(prob_a), _ffi.as_f64p(prob_b),
                                             _KERNEL_TYPES[kernel], gamma, C.byref(handle)))
        self._adopt(handle)


def svc_model(classifier):
    """The device copy of a fitted SVC."""
    return _device_model(SvcModel, classifier)


def svm_predict(classifier, feats, mean, std):
    """Classify every column of feats [n_dims][n_vec] after (x - mean) / std: (classes_ of the winners, probabilities)."""
    m = svc_model(classifier)
    idx, proba = m.predict(feats, mean, std)
    return m.classes[idx], proba


class KnnModel(_DeviceModel):
    """A kNN model on the device (paa_knn_create): callers get class indices.  Reads the classifier's features,
    labels and neighbors, as the reference's Knn.classify does: n_classes = the number of distinct labels, and a label
    that is not one of the integers 0..n_classes-1 is counted for no class."""
    _family = "knn"
    _extra = ("k", np.int32, _ffi.c_i32p)

    def __init__(self, classifier):
        train = np.ascontiguousarray(classifier.features, dtype=np.float64)
        raw = np.asarray(classifier.labels).reshape(-1)
        if train.ndim != 2 or raw.shape[0] != train.shape[0]:
            raise ValueError("kNN model: features %s and %d labels" % (train.shape, raw.shape[0]))
        self.n_classes = int(np.unique(raw).shape[0])
        labels = _class_indices(raw, self.n_classes)
        self.k = int(classifier.neighbors)
        self.n_dims = train.shape[1]
        handle = C.c_void_p()
        _ffi.check(_ffi.lib().paa_knn_create(_ffi.as_f64p(train), _ffi.as_i32p(labels), train.shape[0], self.n_dims,
                                             self.n_classes, self.k, C.byref(handle)))
        self._adopt(handle)

    def predict(self, feats, mean, std, neighbors=False):
        """_DeviceModel.predict; neighbors: also the neighbour indices [n_vec][k] in ascending (squared distance, index)."""
        return super().predict(feats, mean, std, neighbors)


class Knn:
    """The reference's k-nearest-neighbour classifier (audioTrainTest.py:33-49); classify runs on the GPU."""

    def __init__(self, features, labels, neighbors):
        self.features = features
        self.labels = labels
        self.neighbors = neighbors

    def classify(self, test_sample):
        """(first arg-max of P, P) of one feature vector: P[c] = the share of the `neighbors` nearest training rows
        labelled c (divided by `neighbors` also when there are fewer rows)."""
        x = np.asarray(test_sample, dtype=np.float64).reshape(-1, 1)
        idx, proba = knn_model(self).predict(x, np.zeros(x.shape[0]), np.ones(x.shape[0]))     # (x - 0) / 1 == x
        return idx[0], proba[0]


def is_knn(classifier):
    """A kNN classifier: this package's Knn / KnnModel, or any object with the reference Knn's attributes."""
    return isinstance(classifier, (Knn, KnnModel)) or all(hasattr(classifier, a) for a in ("features", "labels", "neighbors"))


def knn_model(classifier):
    """The device copy of a kNN classifier."""
    return _device_model(KnnModel, classifier)


def knn_predict(classifier, feats, mean, std):
    """Classify every column of feats [n_dims][n_vec] after (x - mean) / std with a kNN model: (class indices, P)."""
    return knn_model(classifier).predict(feats, mean, std)


def load_model_knn(knn_model_name, is_regression=False):
    """Loads a kNN model (reference :492-520): eleven pickles -- features, labels, mean, std, class names (not when
    is_regression), neighbors, mid / short windows and steps, compute_beat."""
    with open(knn_model_name, "rb") as fo:
        features = cPickle.load(fo)
        labels = cPickle.load(fo)
        mean = cPickle.load(fo)
        std = cPickle.load(fo)
        if not is_regression:
            classes = cPickle.load(fo)
        neighbors = cPickle.load(fo)
        mid_window = cPickle.load(fo)
        mid_step = cPickle.load(fo)
        short_window = cPickle.load(fo)
        short_step = cPickle.load(fo)
        compute_beat = cPickle.load(fo)

    features = np.array(features)
    labels = np.array(labels)
    mean = np.array(mean)
    std = np.array(std)

    classifier = Knn(features, labels, neighbors)
    if is_regression:
        return classifier, mean, std, mid_window, mid_step, short_window, short_step, compute_beat
    return classifier, mean, std, classes, mid_window, mid_step, short_window, short_step, compute_beat


def _load(model_name, model_type):
    return load_model_knn(model_name) if model_type == "knn" else load_model(model_name)


def device_model(classifier, model_type=None):
    """The device model that serves (classifier, model_type): "knn", a tree-ensemble type, else an SVM; None takes the
    object's kind (is_knn / is_forest)."""
    if model_type == "knn" or (model_type is None and is_knn(classifier)):
        return knn_model(classifier)
    if model_type in _FOREST_TYPES or (model_type is None and is_forest(classifier)):
        return forest_model(classifier)
    return svc_model(classifier)


def predict(classifier, model_type, feats, mean, std):
    """classifier_wrapper for every column of feats [n_dims][n_vec] after (x - mean) / std, in one launch: "knn" gives
    (class indices, P), the SVM and tree-ensemble types (classes_ of the winners, probabilities)."""
    m = device_model(classifier, model_type)
    idx, proba = m.predict(feats, mean, std)
    return m.labels(idx), proba


class ForestArrays:
    """A fitted tree ensemble given as plain arrays (e.g. from an .npz), so that no scikit-learn is needed: kind "averaged"
    (RandomForestClassifier / ExtraTreesClassifier: value [nodes][n_classes], the class fractions of tree_.value) or
    "boosted" (GradientBoostingClassifier: value [nodes], trees stage-major, n_outputs = 1 for two classes, else
    n_classes; init [n_outputs] the constant initial raw score) or "regressor" (RandomForestRegressor: value [nodes], one
    output, classes ignored).  Trees are concatenated: tree t owns nodes
    node_offsets[t] .. node_offsets[t + 1] - 1, and its children_left / children_right / feature index are local to it, in
    scikit-learn's tree_ arrays' terms (-1 children: a leaf)."""

    def __init__(self, kind, node_offsets, children_left, children_right, feature, threshold, missing_go_to_left, value,
                 classes, n_dims, learning_rate=0.0, init=None):
        if kind not in _FOREST_KINDS:
            raise ValueError("tree ensemble kind %r: 'averaged', 'boosted' or 'regressor'" % (kind,))
        self.kind = kind
        self.node_offsets = np.ascontiguousarray(node_offsets, dtype=np.int64)
        self.children_left = np.ascontiguousarray(children_left, dtype=np.int64)
        self.children_right = np.ascontiguousarray(children_right, dtype=np.int64)
        self.feature = np.ascontiguousarray(feature, dtype=np.int64)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        n = self.threshold.shape[0]
        self.missing_go_to_left = np.ascontiguousarray(np.zeros(n) if missing_go_to_left is None else missing_go_to_left,
                                                       dtype=np.uint8)
        self.value = np.ascontiguousarray(value, dtype=np.float64)
        self.classes_ = np.zeros(1) if kind == "regressor" else np.asarray(classes)      # a regressor: one output
        self.n_dims = int(n_dims)
        self.learning_rate = float(learning_rate)
        self.init = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(-1)

    @property
    def n_classes(self):
        return int(self.classes_.shape[0])

    @property
    def n_outputs(self):
        return 1 if self.kind == "boosted" and self.n_classes == 2 else self.n_classes


def _tree_arrays(trees, width):
    """Concatenated tree_ arrays of fitted scikit-learn trees (value rows of `width`)."""
    parts = [t.tree_ for t in trees]
    offsets = np.concatenate([[0], np.cumsum([p.node_count for p in parts])]).astype(np.int64)
    cat = lambda get: np.concatenate([np.asarray(get(p)) for p in parts])          # noqa: E731
    missing = cat(lambda p: getattr(p, "missing_go_to_left", np.zeros(p.node_count, dtype=np.uint8)))
    value = cat(lambda p: np.asarray(p.value, dtype=np.float64).reshape(p.node_count, -1)[:, :width])
    return offsets, cat(lambda p: p.children_left), cat(lambda p: p.children_right), cat(lambda p: p.feature), \
        cat(lambda p: p.threshold), missing, value


def forest_arrays(classifier):
    """ForestArrays of a fitted RandomForestClassifier, ExtraTreesClassifier or GradientBoostingClassifier (only its
    estimators_' tree_ arrays, classes_, n_features_in_ and, boosted, learning_rate and init_ are read), or of a fitted
    RandomForestRegressor (estimators_ and no classes_; one output)."""
    if isinstance(classifier, ForestArrays):
        return classifier
    est = classifier.estimators_
    if not hasattr(classifier, "classes_"):
        if getattr(classifier, "n_outputs_", 1) != 1:
            raise NotImplementedError("multi-output forests are not served by the GPU path")
        arrays = _tree_arrays(list(est), 1)
        return ForestArrays("regressor", *arrays[:6], arrays[6][:, 0], None, int(classifier.n_features_in_))
    classes = np.asarray(classifier.classes_)
    n_dims = int(classifier.n_features_in_)
    if isinstance(est, np.ndarray) and est.ndim == 2:                 # GradientBoostingClassifier: [n_stages][n_outputs]
        init_ = classifier.init_
        if isinstance(init_, str) and init_ == "zero":
            init = np.zeros(est.shape[1])
        elif type(init_).__name__ == "DummyClassifier" and getattr(init_, "strategy", None) == "prior":
            init = np.asarray(classifier._raw_predict_init(np.zeros((1, n_dims), dtype=np.float32)), dtype=np.float64)[0]
        else:
            raise NotImplementedError("gradient boosting with init=%r: the GPU path serves the default prior and 'zero'"
                                      % (init_,))
        arrays = _tree_arrays([e for stage in est for e in stage], 1)
        boosted = ForestArrays("boosted", *arrays[:6], arrays[6][:, 0], classes, n_dims, classifier.learning_rate, init)
        if hasattr(init_, "class_prior_"):                            # (to_sklearn_boosting rebuilds init_ from it)
            boosted.class_prior_ = np.asarray(init_.class_prior_, dtype=np.float64)
        return boosted
    if getattr(classifier, "n_outputs_", 1) != 1:
        raise NotImplementedError("multi-output forests are not served by the GPU path")
    arrays = _tree_arrays(list(est), classes.shape[0])
    return ForestArrays("averaged", *arrays, classes, n_dims)


class ForestModel(_DeviceModel):
    """A tree ensemble on the device (paa_forest_create, which validates and re-lays every tree in preorder)."""
    _family = "forest"
    _extra = ("n_outputs", np.float64, _ffi.c_f64p)

    def __init__(self, classifier):
        a = forest_arrays(classifier)
        self.classes = a.classes_
        self.n_classes = a.n_classes
        self.n_outputs = a.n_outputs
        self.n_dims = a.n_dims
        self.boosted = a.kind == "boosted"
        self.regressor = a.kind == "regressor"
        n_trees = a.node_offsets.shape[0] - 1
        n_nodes = a.threshold.shape[0]
        width = 1 if self.boosted or self.regressor else self.n_classes
        for name in ("children_left", "children_right", "feature", "missing_go_to_left"):
            if getattr(a, name).shape != (n_nodes,):
                raise ValueError("tree ensemble: %s has shape %s for %d nodes" % (name, getattr(a, name).shape, n_nodes))
        if a.value.reshape(n_nodes, -1).shape[1] != width or a.value.size != n_nodes * width or n_trees < 1 \
                or a.node_offsets[-1] != n_nodes:
            raise ValueError("tree ensemble: inconsistent arrays (%d trees, %d nodes, value %s)" % (n_trees, n_nodes,
                                                                                                   a.value.shape))
        init = a.init if self.boosted else np.zeros(1)
        if self.boosted and (init is None or init.shape[0] != self.n_outputs):
            raise ValueError("boosted ensemble: init of %s values for %d outputs" % (
                None if init is None else init.shape[0], self.n_outputs))
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)                       # noqa: E731
        handle = C.c_void_p()
        _ffi.check(_ffi.lib().paa_forest_create(_FOREST_KINDS[a.kind], n_trees, ptr(a.node_offsets), ptr(a.children_left),
                                                ptr(a.children_right), ptr(a.feature), _ffi.as_f64p(a.threshold),
                                                ptr(a.missing_go_to_left), _ffi.as_f64p(a.value), self.n_classes, self.n_dims,
                                                a.learning_rate, _ffi.as_f64p(np.ascontiguousarray(init)), C.byref(handle)))
        self._adopt(handle)

    @staticmethod
    def _raise_invalid(idx):
        """scikit-learn's input validation, for the whole call: NaN (boosted) before infinity."""
        if np.any(idx == -2):
            raise ValueError("Input X contains NaN.")
        if np.any(idx == -1):
            raise ValueError("Input X contains infinity or a value too large for dtype('float32').")

    def predict(self, feats, mean, std, raw=False):
        """_DeviceModel.predict; raw: also the raw tree sums [n_vec][n_outputs] (averaged: before the division by the number
        of trees; boosted: the decision function)."""
        return super().predict(feats, mean, std, raw)


def is_forest(classifier):
    """A tree-ensemble CLASSIFIER: ForestArrays / ForestModel, or a fitted scikit-learn ensemble (estimators_ and
    classes_); a regressor (no classes_, kind "regressor") is not one."""
    if isinstance(classifier, ForestArrays):
        return classifier.kind != "regressor"
    if isinstance(classifier, ForestModel):
        return not classifier.regressor
    return hasattr(classifier, "estimators_") and hasattr(classifier, "classes_")


def forest_model(classifier):
    """The device copy of a fitted tree ensemble."""
    return _device_model(ForestModel, classifier)


def forest_predict(classifier, feats, mean, std):
    """Classify every column of feats [n_dims][n_vec] after (x - mean) / std with a tree ensemble: (classes_ of the
    predictions, predict_proba)."""
    m = forest_model(classifier)
    idx, proba = m.predict(feats, mean, std)
    return m.classes[idx], proba


def load_model(model_name, is_regression=False):
    """Loads an SVM model either for classification or regression (reference :523-553): the pickled classifier and its
    MEANS file (mean, std, class names, mid / short windows and steps, compute_beat)."""
    with open(model_name + "MEANS", "rb") as fo:
        mean = cPickle.load(fo)
        std = cPickle.load(fo)
        if not is_regression:
            classNames = cPickle.load(fo)
        mid_window = cPickle.load(fo)
        mid_step = cPickle.load(fo)
        short_window = cPickle.load(fo)
        short_step = cPickle.load(fo)
        compute_beat = cPickle.load(fo)

    mean = np.array(mean)
    std = np.array(std)

    with open(model_name, 'rb') as fid:
        svm_model = cPickle.load(fid)

    if is_regression:
        return svm_model, mean, std, mid_window, mid_step, short_window, short_step, compute_beat
    return svm_model, mean, std, classNames, mid_window, mid_step, short_window, short_step, compute_beat


def classifier_wrapper(classifier, classifier_type, test_sample):
    """(class id, probability estimate) of one feature vector (reference :52-94).  "svm" / "svm_rbf": predict() and
    predict_proba() on the GPU; "knn": Knn.classify on the GPU (the class INDEX and P); "randomforest" / "extratrees" /
    "gradientboosting": predict() and predict_proba() on the GPU (classes_ and the probabilities); any other type gives
    the reference's (-1, -1)."""
    if classifier_type not in _SVM_TYPES + _FOREST_TYPES + ("knn",):
        return -1, -1
    x = np.asarray(test_sample, dtype=np.float64).reshape(-1, 1)
    m = device_model(classifier, classifier_type)
    idx, proba = m.predict(x, np.zeros(x.shape[0]), np.ones(x.shape[0]))       # (x - 0) / 1 == x
    return m.labels(idx[0]), proba[0]


def _long_term_vector(signal, sampling_rate, mid_window, mid_step, short_window, short_step, compute_beat):
    """file_classification's feature vector (reference :1077-1090): short-file mid_window clamp, long-term mean of the
    mid-term matrix, beat and its confidence appended when compute_beat."""
    if signal.shape[0] / float(sampling_rate) < mid_window:
        mid_window = signal.shape[0] / float(sampling_rate)
    mid_features, s, _ = aF.mid_feature_extraction(signal, sampling_rate, mid_window * sampling_rate,
                                                   mid_step * sampling_rate, round(sampling_rate * short_window),
                                                   round(sampling_rate * short_step))
    mid_features = mid_features.mean(axis=1)
    if compute_beat:
        beat, beat_conf = aF.beat_extraction(s, short_step)
        mid_features = np.append(mid_features, beat)
        mid_features = np.append(mid_features, beat_conf)
    return mid_features


def _long_term_vectors(signals, fs, mid_window, mid_step, short_window, short_step, compute_beat, clamp_short):
    """The long-term vectors [n_dims][n_signals] of many mono signals of one sampling rate: the clips go through ONE batched
    mid-term (+ beat) plan per sample type.  clamp_short: clips shorter than mid_window take file_classification's clamp
    (a window of their own length) through the single-clip path."""
    vectors = [None] * len(signals)
    by_kind = {}
    for i, s in enumerate(signals):
        if not clamp_short or s.shape[0] / float(fs) >= mid_window:
            by_kind.setdefault(np.asarray(s).dtype == np.int16, []).append(i)
    for _, members in by_kind.items():
        mids, beats = aF.mid_and_beat_batch([signals[i] for i in members], fs, mid_window * fs, mid_step * fs,
                                            round(fs * short_window), round(fs * short_step),
                                            beat_window_seconds=short_step if compute_beat else None)
        for j, i in enumerate(members):
            v = mids[j].mean(axis=1)
            if compute_beat:
                v = np.append(v, beats[j, 0])
                v = np.append(v, beats[j, 1])
            vectors[i] = v
    for i, v in enumerate(vectors):
        if v is None:
            vectors[i] = _long_term_vector(signals[i], fs, mid_window, mid_step, short_window, short_step, compute_beat)
    return np.stack(vectors, axis=1)


def file_classification_signal(signal, sampling_rate, classifier, mean, std, mid_window, mid_step, short_window,
                               short_step, compute_beat, model_type="svm_rbf"):
    """file_classification on a mono signal and a loaded model: (class id, probabilities)."""
    mid_features = _long_term_vector(signal, sampling_rate, mid_window, mid_step, short_window, short_step, compute_beat)
    feature_vector = (mid_features - mean) / std    # normalization (:1091)
    return classifier_wrapper(classifier, model_type, feature_vector)


def file_classification(input_file, model_name, model_type):
    """(class id, probabilities, class names) of one audio file (reference :1052-1096); the reference's error returns
    (-1, -1, -1) for a missing model or file and an unreadable file."""
    if not os.path.isfile(model_name):
        print("fileClassification: input model_name not found!")
        return -1, -1, -1
    if isinstance(input_file, str) and not os.path.isfile(input_file):
        print("fileClassification: wav file not found!")
        return -1, -1, -1
    classifier, mean, std, classes, mid_window, mid_step, short_window, short_step, compute_beat = \
        _load(model_name, model_type)
    sampling_rate, signal = audioBasicIO.read_audio_file(input_file)
    signal = audioBasicIO.stereo_to_mono(signal)
    if sampling_rate == 0:
        return -1, -1, -1
    class_id, probability = file_classification_signal(signal, sampling_rate, classifier, mean, std, mid_window, mid_step,
                                                       short_window, short_step, compute_beat, model_type)
    return class_id, probability, classes


def file_classification_signals(signals, sampling_rate, classifier, mean, std, mid_window, mid_step, short_window,
                                short_step, compute_beat, model_type="svm_rbf"):
    """file_classification for many mono signals of one sampling rate and an SVM, kNN or tree-ensemble model: the clips
    go through ONE batched mid-term (+ beat) plan, the long-term vectors through ONE classifier launch.  Clips shorter than mid_window take
    the reference's clamp (:1077-1078, a window of their own length) through the single-clip path.
    Returns (class ids [n], probabilities [n][k])."""
    if len(signals) == 0:
        return np.array([]), np.zeros((0, 0))
    feats = _long_term_vectors(signals, sampling_rate, mid_window, mid_step, short_window, short_step, compute_beat, True)
    return predict(classifier, model_type, feats, mean, std)


def _read_by_sampling_rate(files, indices):
    """{sampling rate: [(index, mono signal), ...]} of files[i] for i in `indices`, taken one by one (a generator may
    announce the files it leaves out between the reads); unreadable files are left out."""
    groups = {}
    for i in indices:
        fs, sig = audioBasicIO.read_audio_file(files[i])
        if fs == 0:
            continue
        groups.setdefault(fs, []).append((i, audioBasicIO.stereo_to_mono(sig)))
    return groups


def file_classification_batch(files, model_name, model_type):
    """file_classification over many files with one model: returns a list of (class id, probabilities, class names)
    per file, equal to one-file calls.  Files are grouped by sampling rate; each group is one batched mid-term plan and
    one classifier launch.  Missing / unreadable files give the reference's (-1, -1, -1)."""
    if model_type not in _SVM_TYPES + _FOREST_TYPES + ("knn",):
        return [file_classification(f, model_name, model_type) for f in files]
    if not os.path.isfile(model_name):
        print("fileClassification: input model_name not found!")
        return [(-1, -1, -1) for _ in files]
    classifier, mean, std, classes, mid_window, mid_step, short_window, short_step, compute_beat = \
        _load(model_name, model_type)
    out = [(-1, -1, -1)] * len(files)

    def present():
        for i, f in enumerate(files):
            if isinstance(f, str) and not os.path.isfile(f):
                print("fileClassification: wav file not found!")
            else:
                yield i
    for fs, members in _read_by_sampling_rate(files, present()).items():
        ids, proba = file_classification_signals([s for _, s in members], fs, classifier, mean, std, mid_window, mid_step,
                                                 short_window, short_step, compute_beat, model_type)
        for j, (i, _) in enumerate(members):
            out[i] = (ids[j], proba[j], classes)
    return out


# ---------------------------------------------------------------------------------------------------------
# regression (reference :96-111, :222-233, :370-489, :774-855, :1099-1151)
# ---------------------------------------------------------------------------------------------------------
class SvrArrays:
    """A fitted epsilon-SVR given by its arrays in scikit-learn's attribute names (e.g. from an .npz): support_vectors
    [n_sv][n_dims] (n_sv = 0 is legal: the model predicts its intercept), dual_coef the PRIVATE _dual_coef_ [1][n_sv],
    intercept the PRIVATE _intercept_ (libsvm's -rho), gamma the fitted _gamma, kernel 'linear' or 'rbf'."""

    def __init__(self, support_vectors, dual_coef, intercept, gamma, kernel):
        self.kernel = _svr_kernel(kernel)
        self.support_vectors_ = np.asarray(support_vectors, dtype=np.float64)
        self._dual_coef_ = np.asarray(dual_coef, dtype=np.float64).reshape(1, -1)
        self._intercept_ = np.asarray(intercept, dtype=np.float64).reshape(-1)
        self._gamma = float(gamma)


def _svr_kernel(kernel):
    kernel = str(kernel)
    if kernel not in _KERNEL_TYPES:
        raise NotImplementedError("SVR kernel %r: the GPU path serves 'rbf' and 'linear' models" % (kernel,))
    return kernel


def _stats_rows(stats, n_models, n_dims, what):
    """[n_models][n_dims] from one vector (shared by every model) or one row per model."""
    a = np.asarray(stats, dtype=np.float64)
    if a.ndim == 1 or (a.ndim == 2 and a.shape[0] == 1 and n_models != 1):
        a = np.broadcast_to(a.reshape(1, -1), (n_models, a.size))
    if a.shape != (n_models, n_dims):
        raise ValueError("%s of shape %s for %d models of %d dims" % (what, a.shape, n_models, n_dims))
    return np.ascontiguousarray(a)


class SvrBank:
    """A bank of fitted SVR models (sklearn.svm.SVR or SvrArrays) that share n_dims, on the device (paa_svr_create), each
    with its own standardisation: means / stds are one row per model, or one vector shared by all of them."""

    def __init__(self, models, means, stds):
        models = list(models)
        if not models:
            raise ValueError("an SVR bank needs at least one model")
        svs, coefs, rho, kernels, gammas = [], [], [], [], []
        for m in models:
            kernel = _svr_kernel(getattr(m, "kernel", ""))
            sv = np.asarray(m.support_vectors_, dtype=np.float64)
            coef = np.asarray(m._dual_coef_, dtype=np.float64).reshape(-1)
            icpt = np.asarray(m._intercept_, dtype=np.float64).reshape(-1)
            if sv.ndim != 2 or coef.shape[0] != sv.shape[0] or icpt.shape[0] != 1:
                raise ValueError("not a fitted SVR: inconsistent arrays")
            svs.append(sv)
            coefs.append(coef)
            rho.append(-icpt[0])
            kernels.append(_KERNEL_TYPES[kernel])
            gammas.append(float(m._gamma) if kernel == "rbf" else 0.0)
        self.n_models = len(models)
        self.n_dims = int(svs[0].shape[1])
        if any(sv.shape[1] != self.n_dims for sv in svs):
            raise ValueError("the models of an SVR bank must share the number of dims")
        self.means = _stats_rows(means, self.n_models, self.n_dims, "means")
        self.stds = _stats_rows(stds, self.n_models, self.n_dims, "stds")
        offsets = np.concatenate([[0], np.cumsum([sv.shape[0] for sv in svs])]).astype(np.int64)
        sv = np.ascontiguousarray(np.concatenate(svs, axis=0))
        coef = np.ascontiguousarray(np.concatenate(coefs))
        handle = C.c_void_p()
        _ffi.check(_ffi.lib().paa_svr_create(
            self.n_models, _ffi.as_i64p(offsets), _ffi.as_f64p(sv) if sv.size else None, _ffi.as_f64p(coef) if coef.size else None,
            _ffi.as_f64p(np.array(rho, dtype=np.float64)), np.array(kernels, dtype=np.int32).ctypes.data_as(_ffi.c_i32p),
            _ffi.as_f64p(np.array(gammas, dtype=np.float64)), _ffi.as_f64p(self.means), _ffi.as_f64p(self.stds), self.n_dims,
            C.byref(handle)))
        self.handle = handle
        self._finalizer = weakref.finalize(self, _ffi.lib().paa_svr_destroy, handle)

    def predict(self, feats):
        """feats [n_dims][n_vec] (feature-major) -> [n_models][n_vec]: model m's prediction of (feats[:, v] - means[m]) / stds[m]."""
        F = np.ascontiguousarray(feats, dtype=np.float64)
        if F.ndim != 2 or F.shape[0] != self.n_dims or F.shape[1] < 1:
            raise ValueError("feature matrix of shape %s for a model of %d dims" % (F.shape, self.n_dims))
        n = F.shape[1]
        out = np.empty((self.n_models, n), dtype=np.float64)
        _ffi.check(_ffi.lib().paa_svr_predict_f64(self.handle, _ffi.as_f64p(F), self.n_dims, n, n, _ffi.as_f64p(out)))
        return out

    def predict_device(self, d_feats, ld, n_vec, d_out=None, ld_out=None):
        """The same on a device-resident matrix (a DeviceBuffer holding [n_dims][ld] doubles).  With d_out (a DeviceBuffer
        of [n_models][ld_out] doubles) the predictions stay on the device and None is returned."""
        if d_out is not None:
            _ffi.check(_ffi.lib().paa_svr_dev_predict_f64(self.handle, d_feats.ptr, self.n_dims, ld, n_vec, d_out.ptr,
                                                          n_vec if ld_out is None else ld_out))
            return None
        buf = _ffi.DeviceBuffer(8 * n_vec * self.n_models)
        try:
            _ffi.check(_ffi.lib().paa_svr_dev_predict_f64(self.handle, d_feats.ptr, self.n_dims, ld, n_vec, buf.ptr, n_vec))
            return buf.to_host(np.float64, n_vec * self.n_models).reshape(self.n_models, n_vec)
        finally:
            buf.free()


def svr_bank(models, means, stds):
    """The device bank of (models, means, stds).  A bank of ONE model is kept while the model lives, like the classifiers'
    device models (and uploaded again when it is asked for with another mean / std)."""
    if isinstance(models, SvrBank):
        return models
    models = list(models)
    if len(models) != 1:
        return SvrBank(models, means, stds)

    def same_stats(b):
        return b.means.shape[1] == np.size(means) == np.size(stds) and \
            np.array_equal(b.means[0], np.asarray(means, dtype=np.float64).reshape(-1)) and \
            np.array_equal(b.stds[0], np.asarray(stds, dtype=np.float64).reshape(-1))
    return _device_model(SvrBank, models[0], lambda m: SvrBank([m], means, stds), same_stats)


def regress(models, model_type, feats, means, stds):
    """regression_wrapper for every model of `models` on every column of feats [n_dims][n_vec], model m after
    (x - means[m]) / stds[m] (one mean / std vector: shared by all): [n_models][n_vec].  "svm" / "svm_rbf": ONE launch
    for the whole bank; "randomforest": one traversal / reduction pair per forest."""
    if model_type in _SVM_TYPES:
        return svr_bank(models, means, stds).predict(feats)
    if model_type != "randomforest":
        raise NotImplementedError("regression model type %r: the GPU path serves 'svm', 'svm_rbf' and 'randomforest'" % (model_type,))
    models = list(models)
    F = np.ascontiguousarray(feats, dtype=np.float64)
    means = _stats_rows(means, len(models), F.shape[0], "means")
    stds = _stats_rows(stds, len(models), F.shape[0], "stds")
    out = np.empty((len(models), F.shape[1]), dtype=np.float64)
    for i, m in enumerate(models):
        out[i] = _forest_regressor(m).predict(F, means[i], stds[i])[1][:, 0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# training and tuning of classifiers (reference :117-219, :236-361, :556-771, :858-911)
# ---------------------------------------------------------------------------------------------------------------------
_CLASSIFIER_TYPES = _SVM_TYPES + ("knn",) + _FOREST_TYPES


def train_knn(features, labels, neighbors):
    """This package's Knn over the given rows (reference :117-129): a kNN has no fit."""
    return Knn(features, labels, neighbors)


def train_svm(features, labels, c_param, kernel='linear'):
    """A fitted sklearn.svm.SVC(probability=True, gamma='auto') (reference :132-155); scikit-learn fits."""
    import sklearn.svm
    svm = sklearn.svm.SVC(C=c_param, kernel=kernel, probability=True, gamma='auto')
    svm.fit(features, labels)
    return svm


def train_random_forest(features, labels, n_estimators):
    """A fitted RandomForestClassifier (reference :158-178); scikit-learn fits."""
    import sklearn.ensemble
    rf = sklearn.ensemble.RandomForestClassifier(n_estimators=n_estimators)
    rf.fit(features, labels)
    return rf


def train_gradient_boosting(features, labels, n_estimators):
    """A fitted GradientBoostingClassifier (reference :181-199); scikit-learn fits."""
    import sklearn.ensemble
    gb = sklearn.ensemble.GradientBoostingClassifier(n_estimators=n_estimators)
    gb.fit(features, labels)
    return gb


def train_extra_trees(features, labels, n_estimators):
    """A fitted ExtraTreesClassifier (reference :202-219); scikit-learn fits."""
    import sklearn.ensemble
    et = sklearn.ensemble.ExtraTreesClassifier(n_estimators=n_estimators)
    et.fit(features, labels)
    return et


def _train_classifier(features, labels, classifier_name, param):
    if classifier_name in _SVM_TYPES:
        return train_svm(features, labels, param, kernel="rbf" if classifier_name == "svm_rbf" else "linear")
    return {"knn": train_knn, "randomforest": train_random_forest, "gradientboosting": train_gradient_boosting,
            "extratrees": train_extra_trees}[classifier_name](features, labels, param)


def features_to_matrix(features):
    """(the feature matrices of a list stacked, the class index of every row as floats) (reference :887-911).  As in the
    reference a list of ONE matrix gives that matrix itself and labels of shape [n][1], an empty list two empty arrays."""
    if len(features) == 0:
        return np.array([]), np.array([])
    if len(features) == 1:
        return features[0], np.zeros((len(features[0]), 1))
    return np.vstack(list(features)), np.concatenate([i * np.ones(len(f)) for i, f in enumerate(features)])


def group_split(X, y, train_indeces, test_indeces, split_id):
    """(X_train, X_test, y_train, y_test) of split `split_id` of two lists of index lists (reference :556-573)."""
    train_index, test_index = train_indeces[split_id], test_indeces[split_id]
    return X[train_index], X[test_index], y[train_index], y[test_index]


def print_confusion_matrix(cm, class_names):
    """Prints a confusion matrix in per cent of all samples (reference :858-884)."""
    if cm.shape[0] != len(class_names):
        print("printConfusionMatrix: Wrong argument sizes\n")
        return
    short = [c[0:3] if len(c) > 4 else c for c in class_names]
    print("".join("\t{0:s}".format(c) for c in short))
    total = np.sum(cm)
    for i, c in enumerate(short):
        print("{0:s}".format(c) + "".join("\t{0:.2f}".format(100.0 * cm[i][j] / total) for j in range(len(class_names))))


def knn_split_geometry():
    """(queries per workgroup, training rows per LDS tile, rows per step, the K instances) of the split-sweep kernel."""
    geo = np.zeros(10, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_debug_knn_split_geometry(geo.ctypes.data_as(_ffi.c_i32p)))
    return int(geo[0]), int(geo[1]), int(geo[2]), tuple(int(v) for v in geo[4:4 + geo[3]])


class _SplitResult:
    def _rows(self, j):
        """job j's rows of every output that has one row per test vector: test_off[j] .. test_off[j + 1] - 1"""
        return slice(int(self.test_off[j]), int(self.test_off[j + 1]))


class KnnSplitResult(_SplitResult):
    """What knn_split_predict returns: label [Q] (int64 class indices), proba [Q][max_classes] or None, neighbors
    [Q][k_launch] or None (train-list positions, -1 past a job's k or train list), test_off [n_jobs + 1] (job j owns the rows
    test_off[j] .. test_off[j + 1] - 1), n_classes [n_jobs] and k [n_jobs]."""

    def __init__(self, label, proba, neighbors, test_off, n_classes, k):
        self.label, self.proba, self.neighbors, self.test_off, self.n_classes, self.k = label, proba, neighbors, test_off, n_classes, k

    def job(self, j):
        """(labels, P [n_test][n_classes_j] or None, neighbours [n_test][k_j] or None) of job j."""
        r = self._rows(j)
        return (self.label[r], None if self.proba is None else self.proba[r, :self.n_classes[j]],
                None if self.neighbors is None else self.neighbors[r, :self.k[j]])


def _index_list(idx, what, j):
    a = np.asarray(idx)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError("job %d: the %s list must be a one-dimensional array of integers" % (j, what))
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError("job %d: a %s index does not fit 32 bits" % (j, what))
    return a.astype(np.int32)


def _offsets(counts):
    """[0, counts[0], counts[0] + counts[1], ...] as int64: list j of a concatenation owns offsets[j] .. offsets[j + 1] - 1."""
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _packed(lists, dtype):       # (the lists as one contiguous array of dtype, their offsets)
    return np.ascontiguousarray(np.concatenate(lists), dtype=dtype), _offsets([a.shape[0] for a in lists])


def _check_kernel(kernel):
    if kernel not in _KERNEL_TYPES:
        raise NotImplementedError("SVM kernel %r: the GPU solver serves 'rbf' and 'linear'" % (kernel,))


_Jobs = collections.namedtuple("_Jobs", "X raw labels train_idx train_off test_idx test_off mean scale last inside")


def _pack_jobs(X, labels, jobs, last, convert, kernel=None):
    """The jobs (train_idx, test_idx, mean, scale, <last>) of a sweep over ONE sample matrix, checked and packed for the library:
    X [n_samples][n_dims] as float64, the raw labels and their int32 class indices, the train and test lists concatenated with
    their offsets [n_jobs + 1], mean / scale [n_jobs][n_dims], per job convert(<last>) and the training rows inside the
    matrix (an index outside is the library's error to report).  kernel: an SVM sweep's, refused before any job is read."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    raw = np.asarray(labels).reshape(-1)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or raw.shape[0] != X.shape[0]:
        raise ValueError("sample matrix of shape %s with %d labels" % (X.shape, raw.shape[0]))
    jobs = list(jobs)
    if not jobs:
        raise ValueError("no jobs")
    if kernel is not None:
        _check_kernel(kernel)
    n_samples, n_dims = X.shape
    train, test, means, scales, lasts, inside = [], [], [], [], [], []
    for j, job in enumerate(jobs):
        if len(job) != 5:
            raise ValueError("job %d: (train_idx, test_idx, mean, scale, %s) expected" % (j, last))
        tr, te = _index_list(job[0], "train", j), _index_list(job[1], "test", j)
        mean, scale = _stats(job[2], job[3], n_dims)
        train.append(tr)
        test.append(te)
        means.append(mean)
        scales.append(scale)
        lasts.append(convert(job[4]))
        inside.append(tr[(tr >= 0) & (tr < n_samples)])
    return _Jobs(X, raw, _class_indices(raw), *_packed(train, np.int32), *_packed(test, np.int32), np.stack(means), np.stack(scales), lasts,
                 inside)


def knn_split_predict(X, labels, jobs, proba=False, neighbors=False):
    """Knn.classify for every job of a sweep over ONE sample matrix, in one launch (paa_knn_splits_f64, knn_split_kernel).
    X [n_samples][n_dims]; labels [n_samples]; a job is (train_idx, test_idx, mean, scale, k): the rows X[train_idx]
    standardised as (x - mean) / scale are the model, in that order, the rows X[test_idx] the queries.  n_classes of a
    job is the number of distinct labels of ITS training rows, as KnnModel counts it (the reference's Knn.classify :40):
    a class absent from a split shrinks it, and rows labelled >= n_classes then vote for no class, like labels that
    are no integers >= 0.  Neighbours rank in ascending (squared distance, position in train_idx).  Returns a KnnSplitResult."""
    p = _pack_jobs(X, labels, jobs, "k", int)
    n_samples, n_dims = p.X.shape
    k = np.array(p.last, dtype=np.int32)
    n_classes = np.array([max(int(np.unique(p.raw[rows]).shape[0]), 1) for rows in p.inside], dtype=np.int32)
    max_classes = int(n_classes.max())
    instances = knn_split_geometry()[3]
    k_launch = min([K for K in instances if K >= int(k.max())], default=instances[-1])
    Q = int(p.test_off[-1])
    label = np.zeros(Q, dtype=np.int32)
    P = np.zeros((Q, max_classes), dtype=np.float64) if proba else None
    nb = np.full((Q, k_launch), -1, dtype=np.int32) if neighbors else None
    _ffi.check(_ffi.lib().paa_knn_splits_f64(
        _ffi.as_f64p(p.X), n_samples, n_dims, _ffi.as_i32p(p.labels), len(k), _ffi.as_i64p(p.train_off), _ffi.as_i32p(p.train_idx),
        _ffi.as_i64p(p.test_off), _ffi.as_i32p(p.test_idx), _ffi.as_f64p(p.mean), _ffi.as_f64p(p.scale), _ffi.as_i32p(k),
        _ffi.as_i32p(n_classes), max_classes, _ffi.as_i32p(label), _ffi.as_f64p(P) if proba else None,
        _ffi.as_i32p(nb) if neighbors else None))
    return KnnSplitResult(label.astype(np.int64), P, nb, p.test_off, n_classes, k)


def smo_geometry():
    """(threads per workgroup, lane groups, rows per task, test rows per scoring workgroup, default iterations per launch,
    dims) of the SMO solver and its scoring kernel (kernels_smo.hpp)."""
    geo = np.zeros(6, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_debug_smo_geometry(geo.ctypes.data_as(_ffi.c_i32p)))
    return tuple(int(v) for v in geo)


SMO_CONVERGED, SMO_NOT_CONVERGED = 2, 3          # PAA_SMO_CONVERGED / PAA_SMO_NOT_CONVERGED
SMO_MAX_ROWS = 8192                              # PAA_SMO_MAX_ROWS


def _warn_not_converged(status, max_iter):
    """scikit-learn's warning for a libsvm fit that stopped at max_iter (its ConvergenceWarning when it is installed)."""
    n = int(np.count_nonzero(np.asarray(status) == SMO_NOT_CONVERGED))
    if not n:
        return
    import warnings
    try:
        from sklearn.exceptions import ConvergenceWarning as category
    except ImportError:
        category = UserWarning
    warnings.warn("Solver terminated early (max_iter=%d) in %d of %d binary problems.  Consider pre-processing your data with "
                  "StandardScaler or MinMaxScaler." % (max_iter, n, len(status)), category, stacklevel=3)


class SmoResult:
    """What smo_solve returns: alpha_y (a list of one array per task, alpha_t y_t in the task's row order), rho, iterations,
    gap and status per task (SMO_CONVERGED / SMO_NOT_CONVERGED) and the number of kernel launches; cached [n_tasks] (bool): the
    task was solved from its group's resident kernel matrix (all False under kernel_cache="none")."""

    def __init__(self, alpha_y, rho, iterations, gap, status, n_launches, cached=None):
        self.alpha_y, self.rho, self.iterations, self.gap, self.status, self.n_launches = alpha_y, rho, iterations, gap, status, n_launches
        self.cached = np.zeros(len(rho), dtype=bool) if cached is None else cached


def _svc_cache_mode(kernel_cache, cache_bytes, device, keyword):
    """_cache_mode for a caller whose SVM fits run on the device only under `keyword`="device": without it kernel_cache and
    cache_bytes must be left at their defaults."""
    cache_bytes_checked = _cache_mode(kernel_cache, cache_bytes)
    if not device and (kernel_cache != "none" or cache_bytes is not None):
        raise ValueError("kernel_cache / cache_bytes are read under %s='device' only" % keyword)
    return cache_bytes_checked


def smo_cache_layout(task_rows, groups, cache_bytes):
    """The layout of the resident kernel matrices of smo_solve(kernel_cache="gram"), restated in plain NumPy (lib_smo.hpp:
    smo_groups_form; the library's own answer is paa_debug_smo_cache_layout).  task_rows: per task its sample indices; groups:
    per task an id, tasks with equal ids form a group (None: every task its own); groups are numbered in order of first
    appearance.  A group's row list is the distinct sample indices of its tasks in order of first appearance over the tasks in
    task order; pos maps every task row to its place in that list (a sample listed twice maps to one place).  The groups'
    matrices, 8 N^2 bytes each, are packed in group order by svr_cache_chunks.  Returns (group_of [n_tasks], the list of the
    groups' row lists, the list of the tasks' pos, chunk [n_groups] from 0 with -1 for a group that is not cached)."""
    task_rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in task_rows]
    ids = list(range(len(task_rows))) if groups is None else [int(g) for g in np.asarray(groups).reshape(-1)]
    if len(ids) != len(task_rows):
        raise ValueError("%d group ids for %d tasks" % (len(ids), len(task_rows)))
    number, group_of, place = {}, [], []
    for g in ids:
        group_of.append(number.setdefault(g, len(number)))
    for _ in number:
        place.append({})
    pos = []
    for rows, g in zip(task_rows, group_of):
        at = place[g]
        pos.append(np.array([at.setdefault(int(r), len(at)) for r in rows], dtype=np.int32))
    group_rows = [np.array(list(at), dtype=np.int32) for at in place]       # a dict keeps insertion order
    return np.array(group_of, dtype=np.int32), group_rows, pos, svr_cache_chunks([len(r) for r in group_rows], cache_bytes)


def smo_solve(X, tasks, kernel="linear", eps=1e-3, max_iter=10**7, iters_per_launch=0, *, kernel_cache="none", cache_bytes=None,
              groups=None):
    """Binary C-SVC dual problems over ONE sample matrix, all solved side by side (paa_smo_tasks_f64, smo_kernel: libsvm's
    Solver without shrinking, FP64).  X [n_samples][n_dims]; a task is (rows, signs, mean, scale, C, gamma): the rows X[rows]
    standardised as (x - mean) / scale, signs +1 (the first class) or -1, gamma read for kernel="rbf" only (None: 1 / n_dims).
    iters_per_launch bounds one kernel launch (0: the library's default); results do not depend on it.  A task that stops at
    max_iter has the status SMO_NOT_CONVERGED and a warning is issued, as scikit-learn does.  kernel_cache="gram" (keyword only)
    solves from resident kernel matrices (paa_smo_tasks_cached_f64, smo_cached_kernel, DESIGN K23) with every output byte-equal
    to kernel_cache="none": groups (one id per task, read under "gram" only; None: every task its own group) names the tasks
    that share one matrix over their distinct rows -- they must have the same mean, scale and gamma, byte for byte; the
    matrices are packed into chunks of at most cache_bytes (None: 4 GiB; see smo_cache_layout), and the tasks of a group whose
    matrix alone exceeds it are solved as under "none" (their `cached` is False).  Returns an SmoResult."""
    cache_bytes = _cache_mode(kernel_cache, cache_bytes)
    X = np.ascontiguousarray(X, dtype=np.float64)
    tasks = list(tasks)
    if groups is not None:
        if cache_bytes is None:
            raise ValueError("groups are read under kernel_cache='gram' only")
        groups = np.ascontiguousarray(np.asarray(groups).reshape(-1), dtype=np.int32)
        if groups.shape[0] != len(tasks):
            raise ValueError("%d group ids for %d tasks" % (groups.shape[0], len(tasks)))
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("sample matrix of shape %s" % (X.shape,))
    if not tasks:
        raise ValueError("no tasks")
    _check_kernel(kernel)
    n_samples, n_dims = X.shape
    rows, signs, means, scales, Cs, gammas = [], [], [], [], [], []
    for t, task in enumerate(tasks):
        if len(task) != 6:
            raise ValueError("task %d: (rows, signs, mean, scale, C, gamma) expected" % t)
        r = _index_list(task[0], "row", t)
        sg = np.asarray(task[1], dtype=np.float64).reshape(-1)
        if sg.shape[0] != r.shape[0]:
            raise ValueError("task %d: %d rows and %d signs" % (t, r.shape[0], sg.shape[0]))
        mean, scale = _stats(task[2], task[3], n_dims)
        rows.append(r)
        signs.append(np.where(sg == 1, 1, np.where(sg == -1, -1, 0)).astype(np.int8))
        means.append(mean)
        scales.append(scale)
        Cs.append(float(task[4]))
        gammas.append(1.0 / n_dims if task[5] is None else float(task[5]))
    idx, off = _packed(rows, np.int32)
    sign = np.ascontiguousarray(np.concatenate(signs), dtype=np.int8)
    mean, scale = np.stack(means), np.stack(scales)
    C_arr, g_arr = np.array(Cs, dtype=np.float64), np.array(gammas, dtype=np.float64)
    n_tasks, total = len(tasks), int(off[-1])
    alpha_y, rho, gap = np.zeros(total), np.zeros(n_tasks), np.zeros(n_tasks)
    iterations, status, launches = np.zeros(n_tasks, dtype=np.int32), np.zeros(n_tasks, dtype=np.int32), np.zeros(1, dtype=np.int32)
    cached = np.zeros(n_tasks, dtype=np.int32)
    args = (_ffi.as_f64p(X), n_samples, n_dims, n_tasks, _ffi.as_i64p(off), _ffi.as_i32p(idx), sign.ctypes.data_as(C.POINTER(C.c_int8)),
            _ffi.as_f64p(mean), _ffi.as_f64p(scale), _ffi.as_f64p(C_arr), _ffi.as_f64p(g_arr), _KERNEL_TYPES[kernel], float(eps),
            int(max_iter), int(iters_per_launch), _ffi.as_f64p(alpha_y), _ffi.as_f64p(rho), _ffi.as_i32p(iterations), _ffi.as_f64p(gap),
            _ffi.as_i32p(status), _ffi.as_i32p(launches))
    if cache_bytes is None:
        _ffi.check(_ffi.lib().paa_smo_tasks_f64(*args))
    else:
        _ffi.check(_ffi.lib().paa_smo_tasks_cached_f64(*args, None if groups is None else _ffi.as_i32p(groups), cache_bytes,
                                                       _ffi.as_i32p(cached)))
    _warn_not_converged(status, int(max_iter))
    return SmoResult([alpha_y[off[t]:off[t + 1]] for t in range(n_tasks)], rho, iterations, gap, status, int(launches[0]), cached != 0)


class SvmSplitResult(_SplitResult):
    """What svm_split_fit_predict returns: label [Q] (class values as in `labels`), decision [Q][max_pairs] or None (zeros past
    a job's pairs), test_off [n_jobs + 1], classes (per job the classes present in its training list, ascending), task_off
    [n_jobs + 1] (job j owns the tasks task_off[j] .. task_off[j + 1] - 1, its pairs (a, b), a < b, row-major) and per task
    iterations, status (SMO_CONVERGED / SMO_NOT_CONVERGED) and n_sv; n_launches of the solver kernel; cached [n_jobs] (bool): the
    job's tasks were solved from its resident kernel matrix (all False under kernel_cache="none")."""

    def __init__(self, label, decision, test_off, classes, task_off, iterations, status, n_sv, n_launches, cached=None):
        self.label, self.decision, self.test_off, self.classes, self.task_off = label, decision, test_off, classes, task_off
        self.iterations, self.status, self.n_sv, self.n_launches = iterations, status, n_sv, n_launches
        self.cached = np.zeros(len(classes), dtype=bool) if cached is None else cached

    def job(self, j):
        """(labels, decision values [n_test][pairs_j] or None, iterations [pairs_j], status [pairs_j], n_sv [pairs_j]) of job j."""
        r = self._rows(j)
        t0, t1 = int(self.task_off[j]), int(self.task_off[j + 1])
        return (self.label[r], None if self.decision is None else self.decision[r, :t1 - t0], self.iterations[t0:t1],
                self.status[t0:t1], self.n_sv[t0:t1])


def svm_split_fit_predict(X, labels, jobs, kernel="linear", gamma=None, eps=1e-3, decision=False, max_iter=10**7, iters_per_launch=0, *,
                          kernel_cache="none", cache_bytes=None):
    """SVC(C, kernel, gamma).fit(train).predict(test) for every job of a sweep over ONE sample matrix (paa_svc_fit_splits_f64:
    every pair of the classes present in a job's training list is a binary problem of smo_kernel, all of them side by side;
    then libsvm's one-against-one vote of every test row).  X [n_samples][n_dims]; labels [n_samples] (integers >= 0 on the
    training rows); a job is (train_idx, test_idx, mean, scale, C).  gamma=None is 1 / n_dims, the reference's gamma='auto'.
    No probabilities are fitted: the sweep reads vote labels only.  kernel_cache and cache_bytes (keyword only) are smo_solve's
    with the JOB as the group: "gram" solves every pair of a job from the job's one resident kernel matrix
    (paa_svc_fit_splits_cached_f64) with byte-equal results.  Returns an SvmSplitResult."""
    cache_bytes = _cache_mode(kernel_cache, cache_bytes)
    p = _pack_jobs(X, labels, jobs, "C", float, kernel)
    n_samples, n_dims = p.X.shape
    classes = [np.unique(p.labels[rows]) for rows in p.inside]
    C_arr = np.array(p.last, dtype=np.float64)
    g_arr = np.full(len(classes), 1.0 / n_dims if gamma is None else float(gamma), dtype=np.float64)
    pairs = [len(c) * (len(c) - 1) // 2 for c in classes]
    task_off = _offsets(pairs)
    n_tasks, max_pairs, Q = int(task_off[-1]), max(max(pairs), 1), int(p.test_off[-1])
    label = np.zeros(Q, dtype=np.int32)
    dec = np.zeros((Q, max_pairs), dtype=np.float64) if decision else None
    iterations, status, n_sv = (np.zeros(max(n_tasks, 1), dtype=np.int32) for _ in range(3))
    launches = np.zeros(1, dtype=np.int32)
    cached = np.zeros(max(len(classes), 1), dtype=np.int32)
    args = (_ffi.as_f64p(p.X), n_samples, n_dims, _ffi.as_i32p(p.labels), len(classes), _ffi.as_i64p(p.train_off), _ffi.as_i32p(p.train_idx),
            _ffi.as_i64p(p.test_off), _ffi.as_i32p(p.test_idx), _ffi.as_f64p(p.mean), _ffi.as_f64p(p.scale), _ffi.as_f64p(C_arr),
            _ffi.as_f64p(g_arr), _KERNEL_TYPES[kernel], float(eps), int(max_iter), int(iters_per_launch), _ffi.as_i32p(label),
            _ffi.as_f64p(dec) if decision else None, max_pairs, n_tasks, _ffi.as_i32p(iterations), _ffi.as_i32p(status), _ffi.as_i32p(n_sv),
            _ffi.as_i32p(launches))
    if cache_bytes is None:
        _ffi.check(_ffi.lib().paa_svc_fit_splits_f64(*args))
    else:
        _ffi.check(_ffi.lib().paa_svc_fit_splits_cached_f64(*args, cache_bytes, _ffi.as_i32p(cached)))
    iterations, status, n_sv = iterations[:n_tasks], status[:n_tasks], n_sv[:n_tasks]
    _warn_not_converged(status, int(max_iter))
    return SvmSplitResult(label.astype(np.int64), dec, p.test_off, classes, task_off, iterations, status, n_sv, int(launches[0]),
                          cached[:len(classes)] != 0)


PLATT_CONVERGED, PLATT_LINE_SEARCH_FAILED, PLATT_MAX_ITERATIONS = 0, 1, 2      # PAA_PLATT_*


def _signs(signs, n, what):
    sg = np.asarray(signs, dtype=np.float64).reshape(-1)
    if sg.shape[0] != n:
        raise ValueError("%s: %d values and %d signs" % (what, n, sg.shape[0]))
    return np.ascontiguousarray(np.where(sg == 1, 1, np.where(sg == -1, -1, 0)), dtype=np.int8)


class PlattResult:
    """What platt_sigmoid returns, per problem: A, B, iterations (Newton iterations) and stop (PLATT_CONVERGED,
    PLATT_LINE_SEARCH_FAILED, PLATT_MAX_ITERATIONS)."""

    def __init__(self, A, B, iterations, stop):
        self.A, self.B, self.iterations, self.stop = A, B, iterations, stop


def platt_sigmoid(dec, signs, offsets):
    """libsvm's sigmoid_train for a batch of problems in one launch (paa_platt_sigmoid_f64, platt_sigmoid_kernel): problem p owns
    the decision values dec[offsets[p] : offsets[p + 1]] with the signs signs[..] (+1: the pair's first class, -1: the second);
    P(first class | dec) = 1 / (1 + exp(A dec + B)).  Returns a PlattResult."""
    dec = np.ascontiguousarray(np.asarray(dec, dtype=np.float64).reshape(-1))
    off = np.ascontiguousarray(np.asarray(offsets).reshape(-1), dtype=np.int64)
    if off.shape[0] < 2:
        raise ValueError("no problems")
    if dec.shape[0] != off[-1]:
        raise ValueError("%d decision values for offsets that end at %d" % (dec.shape[0], off[-1]))
    sign = _signs(signs, dec.shape[0], "platt_sigmoid")
    n = off.shape[0] - 1
    A, B = np.zeros(n), np.zeros(n)
    iterations, stop = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_platt_sigmoid_f64(_ffi.as_f64p(dec), sign.ctypes.data_as(C.POINTER(C.c_int8)), n, _ffi.as_i64p(off),
                                                _ffi.as_f64p(A), _ffi.as_f64p(B), _ffi.as_i32p(iterations), _ffi.as_i32p(stop)))
    return PlattResult(A, B, iterations, stop)


class SvcProbaResult:
    """What svc_fit_proba returns.  classes: per job the classes present in its training list, ascending; pair_off [n_jobs + 1]:
    job j owns the pairs pair_off[j] .. pair_off[j + 1] - 1, its pairs (a, b), a < b, row-major.  Per pair: rows (the sample
    indices in pair-row order: the rows of a in train-list order, then those of b), signs (+1 / -1), alpha_y (the full fit's
    alpha_t y_t over those rows), rho, prob_a, prob_b, n_sv, iterations / status [6] (slot 0: the full fit, 1..5: the folds;
    status 0: the fold made no task), sigmoid_iterations, sigmoid_stop (PLATT_*) and cv_dec (the held-out decision values over
    the rows, or None); n_launches of the solver kernel; cached [n_jobs] (bool): the job's full fits and fold fits were solved
    from its resident kernel matrix (all False under kernel_cache="none")."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _seeds(seeds, n_jobs):
    s = np.asarray(seeds)
    if s.dtype.kind not in "iu" or s.ndim > 1 or (s.ndim == 1 and s.shape[0] != n_jobs):
        raise ValueError("seeds: one integer, or one per job")
    s = np.ascontiguousarray(np.broadcast_to(s.astype(np.int64), (n_jobs,)))
    if (s < 0).any() or (s > np.iinfo(np.int32).max).any():
        raise ValueError("seeds: libsvm's random_seed is in 0 .. 2^31 - 1")
    return s


def svc_fit_proba(X, labels, jobs, kernel="linear", gamma=None, eps=1e-3, seeds=0, return_cv=False, max_iter=10**7, iters_per_launch=0, *,
                  kernel_cache="none", cache_bytes=None):
    """SVC(C, kernel, gamma, probability=True).fit(train) for every job over ONE sample matrix (paa_svc_fit_proba_f64): per pair
    of the classes present in a job the full fit and the fits of libsvm's five cross-validation folds are binary problems of
    smo_kernel, all of them side by side; svc_pairs_kernel scores every fold's held-out rows; one platt_sigmoid_kernel launch
    fits probA / probB of every pair.  X [n_samples][n_dims]; labels [n_samples] (integers >= 0 on the training rows); a job is
    (train_idx, mean, scale, C).  seeds: libsvm's random_seed of every job (what scikit-learn draws from random_state), one int
    for all jobs or one per job; the folds are libsvm's for that seed.  gamma=None is 1 / n_dims.  kernel_cache and cache_bytes
    (keyword only) are smo_solve's with the JOB as the group: under "gram" the full fits and all fold fits of a job read the
    job's one resident kernel matrix (paa_svc_fit_proba_cached_f64) with byte-equal results.  Returns an SvcProbaResult."""
    cache_bytes = _cache_mode(kernel_cache, cache_bytes)
    jobs = list(jobs)
    for j, job in enumerate(jobs):
        if len(job) != 4:
            raise ValueError("job %d: (train_idx, mean, scale, C) expected" % j)
    no_test = np.zeros(0, dtype=np.int32)
    p = _pack_jobs(X, labels, [(job[0], no_test, job[1], job[2], job[3]) for job in jobs], "C", float, kernel)
    n_samples, n_dims = p.X.shape
    seed = _seeds(seeds, len(jobs))
    classes = [np.unique(p.labels[rows]) for rows in p.inside]
    rows, signs = [], []
    for tr, cl in zip(p.inside, classes):
        lab = p.labels[tr]
        for a in range(len(cl)):
            for b in range(a + 1, len(cl)):
                ra, rb = tr[lab == cl[a]], tr[lab == cl[b]]
                rows.append(np.concatenate([ra, rb]))
                signs.append(np.concatenate([np.ones(len(ra), dtype=np.int8), -np.ones(len(rb), dtype=np.int8)]))
    pair_off = _offsets([len(c) * (len(c) - 1) // 2 for c in classes])
    row_off = _offsets([len(r) for r in rows])
    n_pairs, n_rows = len(rows), int(row_off[-1])
    C_arr = np.array(p.last, dtype=np.float64)
    g_arr = np.full(len(jobs), 1.0 / n_dims if gamma is None else float(gamma), dtype=np.float64)
    m = max(n_pairs, 1)
    alpha_y, cv = np.zeros(max(n_rows, 1)), np.zeros(max(n_rows, 1)) if return_cv else None
    rho, prob_a, prob_b = np.zeros(m), np.zeros(m), np.zeros(m)
    n_sv, sig_it, sig_stop = (np.zeros(m, dtype=np.int32) for _ in range(3))
    iterations, status = np.zeros((m, 6), dtype=np.int32), np.zeros((m, 6), dtype=np.int32)
    launches = np.zeros(1, dtype=np.int32)
    cached = np.zeros(max(len(jobs), 1), dtype=np.int32)
    args = (_ffi.as_f64p(p.X), n_samples, n_dims, _ffi.as_i32p(p.labels), len(jobs), _ffi.as_i64p(p.train_off), _ffi.as_i32p(p.train_idx),
            _ffi.as_f64p(p.mean), _ffi.as_f64p(p.scale), _ffi.as_f64p(C_arr), _ffi.as_f64p(g_arr), _KERNEL_TYPES[kernel], float(eps),
            int(max_iter), int(iters_per_launch), _ffi.as_i64p(seed), n_pairs, n_rows, _ffi.as_f64p(alpha_y), _ffi.as_f64p(rho),
            _ffi.as_f64p(prob_a), _ffi.as_f64p(prob_b), _ffi.as_i32p(n_sv), _ffi.as_i32p(iterations), _ffi.as_i32p(status),
            _ffi.as_i32p(sig_it), _ffi.as_i32p(sig_stop), _ffi.as_f64p(cv) if return_cv else None, _ffi.as_i32p(launches))
    if cache_bytes is None:
        _ffi.check(_ffi.lib().paa_svc_fit_proba_f64(*args))
    else:
        _ffi.check(_ffi.lib().paa_svc_fit_proba_cached_f64(*args, cache_bytes, _ffi.as_i32p(cached)))
    _warn_not_converged(status[:n_pairs].reshape(-1), int(max_iter))
    per_pair = lambda a: [a[row_off[t]:row_off[t + 1]] for t in range(n_pairs)]
    return SvcProbaResult(classes=classes, pair_off=pair_off, rows=rows, signs=signs, alpha_y=per_pair(alpha_y), rho=rho[:n_pairs],
                          prob_a=prob_a[:n_pairs], prob_b=prob_b[:n_pairs], n_sv=n_sv[:n_pairs], iterations=iterations[:n_pairs],
                          status=status[:n_pairs], sigmoid_iterations=sig_it[:n_pairs], sigmoid_stop=sig_stop[:n_pairs],
                          cv_dec=per_pair(cv) if return_cv else None, n_launches=int(launches[0]), cached=cached[:len(jobs)] != 0)


class DeviceSvc:
    """What train_svm_device returns: a fitted probabilistic SVC given by its arrays in scikit-learn's attribute names and
    conventions (support_, support_vectors_, n_support_, dual_coef_ / _dual_coef_, intercept_ / _intercept_, probA_, probB_,
    classes_, kernel, _gamma, C; shape_fit_ for to_sklearn_svc).  svc_model, svm_predict, classifier_wrapper, device_model and
    audioSegmentation.svm_onset_probability read it as they read an sklearn.svm.SVC."""
    probability = True
    gamma = "auto"

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _libsvm_seed(random_state):
    """libsvm's random_seed as scikit-learn draws it: check_random_state(random_state).randint(np.iinfo('i').max) -- None is ONE
    draw from NumPy's global state, an int a fresh RandomState, a RandomState itself."""
    if random_state is None:
        return int(np.random.randint(np.iinfo('i').max))
    if isinstance(random_state, np.random.RandomState):
        return int(random_state.randint(np.iinfo('i').max))
    return int(np.random.RandomState(random_state).randint(np.iinfo('i').max))


def _train_svm_device(features, labels, c_param, kernel, random_state, mean, scale, kernel_cache="none", cache_bytes=None):
    """train_svm_device over the rows (features - mean) / scale, standardised on the load path."""
    _cache_mode(kernel_cache, cache_bytes)
    X = np.ascontiguousarray(features, dtype=np.float64)
    raw = np.asarray(labels).reshape(-1)
    if X.ndim != 2 or X.shape[0] < 1 or raw.shape[0] != X.shape[0]:
        raise ValueError("sample matrix of shape %s with %d labels" % (X.shape, raw.shape[0]))
    _check_kernel(kernel)
    classes, y = np.unique(raw, return_inverse=True)
    k = classes.shape[0]
    if k < 2:
        raise ValueError("The number of classes has to be greater than one; got %d class" % k)
    counts = np.bincount(y, minlength=k)
    top = int(np.sort(counts)[-2:].sum())
    if top > SMO_MAX_ROWS:
        raise NotImplementedError("a pair of classes has %d rows: the GPU solver serves at most %d rows per pair" % (top, SMO_MAX_ROWS))
    seed = _libsvm_seed(random_state)
    n, n_dims = X.shape
    res = svc_fit_proba(X, y.astype(np.int32), [(np.arange(n), mean, scale, float(c_param))], kernel=kernel, seeds=seed,
                        kernel_cache=kernel_cache, cache_bytes=cache_bytes)
    # libsvm's model: the support vectors are the union over the pairs, grouped by class ascending, in sample order within a class
    coef = np.zeros((k - 1, n))
    is_sv = np.zeros(n, dtype=bool)
    t = 0
    for a in range(k):
        for b in range(a + 1, k):
            rows, ay = res.rows[t], res.alpha_y[t]
            in_a = y[rows] == a
            coef[b - 1, rows[in_a]] = ay[in_a]           # class a's coefficients against b: row b - 1
            coef[a, rows[~in_a]] = ay[~in_a]             # class b's against a: row a
            is_sv[rows[ay != 0]] = True
            t += 1
    support = np.flatnonzero(is_sv)
    support = support[np.argsort(y[support], kind="stable")].astype(np.int32)
    dual = np.ascontiguousarray(coef[:, support])
    intercept = -res.rho
    flip = -1.0 if k == 2 else 1.0                       # scikit-learn publishes the two-class model negated
    n_support = np.bincount(y[support], minlength=k).astype(np.int32)
    return DeviceSvc(support_=support, support_vectors_=np.ascontiguousarray((X[support] - mean) / scale),
                     n_support_=n_support, _n_support=n_support.copy(), _dual_coef_=dual, dual_coef_=flip * dual, _intercept_=intercept, intercept_=flip * intercept,
                     probA_=res.prob_a.copy(), probB_=res.prob_b.copy(), _probA=res.prob_a.copy(), _probB=res.prob_b.copy(),
                     classes_=classes, kernel=kernel, _gamma=1.0 / n_dims, C=float(c_param), shape_fit_=X.shape, fit_status_=0,
                     n_features_in_=n_dims, random_seed=seed, fit_result=res)


def train_svm_device(features, labels, c_param, kernel='linear', *, random_state=None, kernel_cache="none", cache_bytes=None):
    """train_svm on the GPU: SVC(C=c_param, kernel=kernel, probability=True, gamma='auto', random_state=random_state).fit(features,
    labels) by svc_fit_proba -- every pair's full fit, libsvm's five cross-validation fits per pair for that seed and the
    sigmoid fits.  Returns a DeviceSvc.  random_state=None draws the seed from NumPy's global state exactly as scikit-learn
    does (one randint), an int goes through np.random.RandomState.  A pair of classes above 8192 rows raises
    NotImplementedError; there is no CPU fallback.  Agreement with scikit-learn is bounded by libsvm's stopping tolerance (its
    kernel cache is float32), not bit-exact.  kernel_cache / cache_bytes (keyword only) are svc_fit_proba's: under "gram" every
    pair's full fit and fold fits read ONE resident kernel matrix over all rows, and the model is the same, byte for byte
    (fit_result.cached tells whether the matrix fitted the budget)."""
    _cache_mode(kernel_cache, cache_bytes)
    n_dims = np.asarray(features).shape[1] if np.asarray(features).ndim == 2 else 0
    return _train_svm_device(features, labels, c_param, kernel, random_state, np.zeros(n_dims), np.ones(n_dims), kernel_cache, cache_bytes)


def to_sklearn_svc(model):
    """A real sklearn.svm.SVC with the fitted attributes of a DeviceSvc (or of anything that carries them): it predicts as
    scikit-learn predicts from those arrays and pickles as the reference's model files do.  Needs scikit-learn."""
    import sklearn.svm
    svc = sklearn.svm.SVC(C=float(model.C), kernel=model.kernel, probability=True, gamma='auto')
    n_support = np.asarray(model.n_support_, dtype=np.int32)
    k = n_support.shape[0]
    svc.support_ = np.asarray(model.support_, dtype=np.int32)
    svc.support_vectors_ = np.ascontiguousarray(model.support_vectors_, dtype=np.float64)
    svc._n_support = n_support
    svc._dual_coef_ = np.ascontiguousarray(model._dual_coef_, dtype=np.float64)
    svc._intercept_ = np.ascontiguousarray(model._intercept_, dtype=np.float64)
    flip = -1.0 if k == 2 else 1.0
    svc.dual_coef_ = flip * svc._dual_coef_
    svc.intercept_ = flip * svc._intercept_
    svc._probA = np.ascontiguousarray(model.probA_, dtype=np.float64)
    svc._probB = np.ascontiguousarray(model.probB_, dtype=np.float64)
    svc.classes_ = np.asarray(model.classes_)
    svc._gamma = float(model._gamma)
    svc._sparse = False
    svc.shape_fit_ = tuple(model.shape_fit_)
    svc.fit_status_ = 0
    svc.class_weight_ = np.ones(k)
    svc.n_features_in_ = int(svc.support_vectors_.shape[1])
    return svc


class SvrSolveResult:
    """What svr_solve returns: beta and train_pred (lists of one array per task, in the task's row order: alpha_t - alpha_{t+n}
    and the prediction of the row), rho, iterations, gap, status (SMO_CONVERGED / SMO_NOT_CONVERGED) and n_sv (rows with
    beta != 0) per task and the number of kernel launches; cached [n_tasks] (bool): the task was solved from its resident
    kernel matrix (all False under kernel_cache="none")."""

    def __init__(self, beta, train_pred, rho, iterations, gap, status, n_sv, n_launches, cached=None):
        self.beta, self.train_pred, self.rho, self.iterations, self.gap = beta, train_pred, rho, iterations, gap
        self.status, self.n_sv, self.n_launches = status, n_sv, n_launches
        self.cached = np.zeros(len(rho), dtype=bool) if cached is None else cached


def _targets(y, n_samples):
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    if y.shape[0] != n_samples:
        raise ValueError("%d targets for %d samples" % (y.shape[0], n_samples))
    return y


SVR_CACHE_BYTES = 4 << 30                        # the default budget of kernel_cache="gram": 4 GiB of resident kernel matrices
SVR_GRAM_TILE = 32                               # rows of a tile of svr_gram_kernel (svrfit::kGramTile)


def _cache_mode(kernel_cache, cache_bytes):
    """cache_bytes of a call (None without a cache): kernel_cache is "none" or "gram", cache_bytes None (the default budget)
    or a positive number of bytes, read under "gram" only."""
    if kernel_cache not in ("none", "gram"):
        raise ValueError("kernel_cache=%r: 'none' or 'gram'" % (kernel_cache,))
    if kernel_cache == "none":
        return None
    cache_bytes = SVR_CACHE_BYTES if cache_bytes is None else int(cache_bytes)
    if cache_bytes <= 0:
        raise ValueError("cache_bytes = %d: a positive budget is needed" % cache_bytes)
    return cache_bytes


def svr_cache_chunks(rows, cache_bytes):
    """The packing rule of the resident kernel matrices, restated (lib_gramcache.hpp: svr_cache_pack): rows [n_tasks] are the
    tasks' row counts; the matrix of a task of n rows takes 8 n^2 bytes.  In task order, a task whose matrix exceeds
    cache_bytes is not cached; any other joins the open chunk when the chunk's matrices and its own fit cache_bytes together
    and otherwise opens the next.  Returns the chunk of every task from 0, -1 for a task that is not cached."""
    chunk_of, n_chunks, used = [], 0, 0
    for n in rows:
        size = 8 * int(n) * int(n)
        if size > cache_bytes:
            chunk_of.append(-1)
            continue
        if n_chunks == 0 or used + size > cache_bytes:
            n_chunks, used = n_chunks + 1, 0
        used += size
        chunk_of.append(n_chunks - 1)
    return np.array(chunk_of, dtype=np.int64)


def svr_solve(X, y, tasks, kernel="linear", eps=1e-3, max_iter=10**7, iters_per_launch=0, *, kernel_cache="none", cache_bytes=None):
    """Epsilon-SVR dual problems over ONE sample matrix and its targets, all solved side by side (paa_svr_tasks_f64,
    svr_smo_kernel: libsvm's solve_epsilon_svr over its Solver without shrinking, FP64).  X [n_samples][n_dims]; y [n_samples];
    a task is (rows, mean, scale, C, gamma, epsilon): the rows X[rows] standardised as (x - mean) / scale with the targets
    y[rows], gamma read for kernel="rbf" only (None: 1 / n_dims).  iters_per_launch bounds one kernel launch (0: the library's
    default); results do not depend on it.  A task that stops at max_iter has the status SMO_NOT_CONVERGED and a warning is
    issued, as scikit-learn does.  The prediction for a standardised z is sum_t beta_t K(z_t, z) - rho; train_pred holds it
    for the task's own rows, read from the solver's gradient.  kernel_cache="gram" (keyword only) forms every task's n x n
    kernel matrix once on the device and solves from it (paa_svr_tasks_cached_f64, DESIGN K22): every output is byte-equal to
    kernel_cache="none"; the matrices are packed into chunks of at most cache_bytes (None: 4 GiB; see svr_cache_chunks), and
    a task whose matrix alone exceeds it is solved as under "none" (its `cached` is False).  Returns an SvrSolveResult."""
    cache_bytes = _cache_mode(kernel_cache, cache_bytes)
    X = np.ascontiguousarray(X, dtype=np.float64)
    tasks = list(tasks)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("sample matrix of shape %s" % (X.shape,))
    if not tasks:
        raise ValueError("no tasks")
    _check_kernel(kernel)
    n_samples, n_dims = X.shape
    y = _targets(y, n_samples)
    rows, means, scales, Cs, gammas, epsilons = [], [], [], [], [], []
    for t, task in enumerate(tasks):
        if len(task) != 6:
            raise ValueError("task %d: (rows, mean, scale, C, gamma, epsilon) expected" % t)
        rows.append(_index_list(task[0], "row", t))
        mean, scale = _stats(task[1], task[2], n_dims)
        means.append(mean)
        scales.append(scale)
        Cs.append(float(task[3]))
        gammas.append(1.0 / n_dims if task[4] is None else float(task[4]))
        epsilons.append(float(task[5]))
    idx, off = _packed(rows, np.int32)
    mean, scale = np.stack(means), np.stack(scales)
    C_arr, g_arr, e_arr = (np.array(v, dtype=np.float64) for v in (Cs, gammas, epsilons))
    n_tasks, total = len(tasks), int(off[-1])
    beta, train_pred, rho, gap = np.zeros(total), np.zeros(total), np.zeros(n_tasks), np.zeros(n_tasks)
    iterations, status, n_sv = (np.zeros(n_tasks, dtype=np.int32) for _ in range(3))
    launches = np.zeros(1, dtype=np.int32)
    cached = np.zeros(n_tasks, dtype=np.int32)
    args = (_ffi.as_f64p(X), n_samples, n_dims, _ffi.as_f64p(y), n_tasks, _ffi.as_i64p(off), _ffi.as_i32p(idx), _ffi.as_f64p(mean),
            _ffi.as_f64p(scale), _ffi.as_f64p(C_arr), _ffi.as_f64p(g_arr), _ffi.as_f64p(e_arr), _KERNEL_TYPES[kernel], float(eps),
            int(max_iter), int(iters_per_launch), _ffi.as_f64p(beta), _ffi.as_f64p(rho), _ffi.as_i32p(iterations), _ffi.as_f64p(gap),
            _ffi.as_i32p(status), _ffi.as_i32p(n_sv), _ffi.as_f64p(train_pred), _ffi.as_i32p(launches))
    if cache_bytes is None:
        _ffi.check(_ffi.lib().paa_svr_tasks_f64(*args))
    else:
        _ffi.check(_ffi.lib().paa_svr_tasks_cached_f64(*args, cache_bytes, _ffi.as_i32p(cached)))
    _warn_not_converged(status, int(max_iter))
    per_task = lambda a: [a[off[t]:off[t + 1]] for t in range(n_tasks)]
    return SvrSolveResult(per_task(beta), per_task(train_pred), rho, iterations, gap, status, n_sv, int(launches[0]), cached != 0)


def svr_kernel_matrix(X, tasks, kernel, *, with_qd=False):
    """The output of the Gram kernel alone (paa_svr_gram_f64: svr_standardise_kernel, svr_gram_kernel): X [n_samples][n_dims];
    a task is (rows, mean, scale, gamma) (gamma None: 1 / n_dims; read for kernel="rbf" only).  Returns the list of the tasks'
    full kernel matrices [n][n] over their standardised rows; with_qd=True (keyword only) returns (that list, the list of
    K_tt [n] that the recomputing solver forms at a task's start)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    tasks = list(tasks)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("sample matrix of shape %s" % (X.shape,))
    if not tasks:
        raise ValueError("no tasks")
    _check_kernel(kernel)
    n_samples, n_dims = X.shape
    rows, means, scales, gammas = [], [], [], []
    for t, task in enumerate(tasks):
        if len(task) != 4:
            raise ValueError("task %d: (rows, mean, scale, gamma) expected" % t)
        rows.append(_index_list(task[0], "row", t))
        mean, scale = _stats(task[1], task[2], n_dims)
        means.append(mean)
        scales.append(scale)
        gammas.append(1.0 / n_dims if task[3] is None else float(task[3]))
    idx, off = _packed(rows, np.int32)
    sizes = [int(off[t + 1] - off[t]) ** 2 for t in range(len(tasks))]
    K, qd = np.zeros(sum(sizes)), np.zeros(int(off[-1]))
    _ffi.check(_ffi.lib().paa_svr_gram_f64(
        _ffi.as_f64p(X), n_samples, n_dims, len(tasks), _ffi.as_i64p(off), _ffi.as_i32p(idx), _ffi.as_f64p(np.stack(means)),
        _ffi.as_f64p(np.stack(scales)), _ffi.as_f64p(np.array(gammas, dtype=np.float64)), _KERNEL_TYPES[kernel], _ffi.as_f64p(K),
        _ffi.as_f64p(qd) if with_qd else None))
    at = np.concatenate([[0], np.cumsum(sizes)])
    mats = [K[at[t]:at[t + 1]].reshape(int(off[t + 1] - off[t]), -1) for t in range(len(tasks))]
    return (mats, [qd[off[t]:off[t + 1]] for t in range(len(tasks))]) if with_qd else mats


class SvrSplitResult(_SplitResult):
    """What svr_split_fit_predict returns: pred [Q] (the test predictions), train_pred [T] or None (the training predictions,
    job j owns train_off[j] .. train_off[j + 1] - 1), test_off / train_off [n_jobs + 1], gamma [n_jobs] (the values the fits ran
    with) and per job iterations, status (SMO_CONVERGED / SMO_NOT_CONVERGED) and n_sv; n_launches of the solver kernel; cached
    [n_jobs] (bool): the job was solved from its resident kernel matrix (all False under kernel_cache="none")."""

    def __init__(self, pred, train_pred, test_off, train_off, gamma, iterations, status, n_sv, n_launches, cached=None):
        self.pred, self.train_pred, self.test_off, self.train_off, self.gamma = pred, train_pred, test_off, train_off, gamma
        self.iterations, self.status, self.n_sv, self.n_launches = iterations, status, n_sv, n_launches
        self.cached = np.zeros(len(gamma), dtype=bool) if cached is None else cached

    def job(self, j):
        """(test predictions, training predictions or None, iterations, status, n_sv) of job j."""
        t0, t1 = int(self.train_off[j]), int(self.train_off[j + 1])
        return (self.pred[self._rows(j)], None if self.train_pred is None else self.train_pred[t0:t1], int(self.iterations[j]),
                int(self.status[j]), int(self.n_sv[j]))


def svr_split_fit_predict(X, y, jobs, kernel="linear", gamma=None, epsilon=0.1, eps=1e-3, train_pred=False, max_iter=10**7,
                          iters_per_launch=0, *, kernel_cache="none", cache_bytes=None):
    """SVR(C, kernel, gamma, epsilon).fit(train).predict(test) for every job of a sweep over ONE sample matrix
    (paa_svr_fit_splits_f64: every job is one epsilon-SVR problem of svr_smo_kernel, all of them side by side; then the test
    rows of every job are scored).  X [n_samples][n_dims]; y [n_samples]; a job is (train_idx, test_idx, mean, scale, C).
    gamma=None is scikit-learn's SVR default, 'scale': per job 1 / (n_dims * Z.var()) of its standardised training rows Z (1
    when that variance is 0), formed with NumPy on the host.  train_pred=True also returns the predictions of every job's
    training rows, which the solver reads from its final gradient: no training row is scored again.  kernel_cache and
    cache_bytes (keyword only) are svr_solve's: "gram" solves every job from its resident kernel matrix
    (paa_svr_fit_splits_cached_f64) with byte-equal results.  Returns an SvrSplitResult."""
    cache_bytes = _cache_mode(kernel_cache, cache_bytes)
    p = _pack_jobs(X, y, jobs, "C", float, kernel)
    n_samples, n_dims = p.X.shape
    targets = _targets(p.raw, n_samples)
    n_jobs = len(p.last)
    C_arr = np.array(p.last, dtype=np.float64)
    if gamma is None:
        g_arr = np.ones(n_jobs)
        for j, rows in enumerate(p.inside):
            var = ((p.X[rows] - p.mean[j]) / p.scale[j]).var() if kernel == "rbf" and rows.shape[0] else 0.0
            if var != 0:
                g_arr[j] = 1.0 / (n_dims * var)
    else:
        g_arr = np.full(n_jobs, float(gamma), dtype=np.float64)
    e_arr = np.full(n_jobs, float(epsilon), dtype=np.float64)
    Q, T = int(p.test_off[-1]), int(p.train_off[-1])
    pred = np.zeros(Q)
    tp = np.zeros(T) if train_pred else None
    iterations, status, n_sv = (np.zeros(n_jobs, dtype=np.int32) for _ in range(3))
    launches = np.zeros(1, dtype=np.int32)
    cached = np.zeros(n_jobs, dtype=np.int32)
    args = (_ffi.as_f64p(p.X), n_samples, n_dims, _ffi.as_f64p(targets), n_jobs, _ffi.as_i64p(p.train_off), _ffi.as_i32p(p.train_idx),
            _ffi.as_i64p(p.test_off), _ffi.as_i32p(p.test_idx), _ffi.as_f64p(p.mean), _ffi.as_f64p(p.scale), _ffi.as_f64p(C_arr),
            _ffi.as_f64p(g_arr), _ffi.as_f64p(e_arr), _KERNEL_TYPES[kernel], float(eps), int(max_iter), int(iters_per_launch),
            _ffi.as_f64p(pred), _ffi.as_f64p(tp) if train_pred else None, _ffi.as_i32p(iterations), _ffi.as_i32p(status),
            _ffi.as_i32p(n_sv), _ffi.as_i32p(launches))
    if cache_bytes is None:
        _ffi.check(_ffi.lib().paa_svr_fit_splits_f64(*args))
    else:
        _ffi.check(_ffi.lib().paa_svr_fit_splits_cached_f64(*args, cache_bytes, _ffi.as_i32p(cached)))
    _warn_not_converged(status, int(max_iter))
    return SvrSplitResult(pred, tp, p.test_off, p.train_off, g_arr, iterations, status, n_sv, int(launches[0]), cached != 0)


TREE_MAX_ROWS = 8192                             # PAA_TREE_MAX_ROWS: rows of one tree's training list
TREE_MAX_WEIGHT = 8191                           # PAA_TREE_MAX_WEIGHT
RAND_R_MAX = 2147483647                          # scikit-learn's RAND_R_MAX: a splitter's rand_r seed is randint(0, RAND_R_MAX)
_TREE_SPLITTERS = {"best": 0, "random": 1}       # PAA_TREE_BEST / PAA_TREE_RANDOM
_FOREST_FIT_KINDS = {"randomforest": "best", "extratrees": "random"}
_TREE_RS = np.random.RandomState(0)              # tree_inputs' own generator, re-seeded per tree; never NumPy's global state
_TREE_FIELDS = ("children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted_n_node_samples",
                "missing_go_to_left", "value")
_TREE_DTYPES = (np.int32, np.int32, np.int32, np.float64, np.float64, np.int32, np.float64, np.uint8, np.float64)
_AS_POINTER = {np.int32: _ffi.as_i32p, np.float64: _ffi.as_f64p, np.uint8: _ffi.as_u8p}


def tree_fit_geometry():
    """(threads per workgroup, rows per tree, classes, dims, the largest weight, MiB of device scratch per chunk of a sweep) of
    the tree builder (kernels_treefit.hpp)."""
    geo = np.zeros(6, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_debug_tree_fit_geometry(geo.ctypes.data_as(_ffi.c_i32p)))
    return tuple(int(v) for v in geo)


def _tree_outputs(n_trees, total_nodes, total_values):
    """The arrays a library call writes trees to -- (node counts [n_trees], {field: array} by _TREE_FIELDS: value with total_values
    entries, the others one per node; no array is empty) -- and their ten pointers, the tail of the C signatures' tree arguments."""
    count = np.zeros(max(n_trees, 1), dtype=np.int32)
    out = {name: np.zeros(max(total_values if name == "value" else total_nodes, 1), dtype=dtype) for name, dtype in zip(_TREE_FIELDS, _TREE_DTYPES)}
    return count, out, (_ffi.as_i32p(count),) + tuple(_AS_POINTER[dtype](out[name]) for name, dtype in zip(_TREE_FIELDS, _TREE_DTYPES))


def _raise_tree_flags(flags):
    """scikit-learn's input validation of the standardised float32 training rows, for the whole call: NaN before infinity."""
    flags = np.asarray(flags)
    if np.any(flags & 2):
        raise ValueError("Input X contains NaN.")
    if np.any(flags & 1):
        raise ValueError("Input X contains infinity or a value too large for dtype('float32').")


def _check_tree_rows(n, what):
    if n > TREE_MAX_ROWS:
        raise NotImplementedError("%s has %d training rows: the GPU tree builder serves at most %d rows per tree" % (what, n, TREE_MAX_ROWS))


def _check_targets(y):
    """scikit-learn's validation of regression targets: NaN before infinity."""
    y = np.asarray(y, dtype=np.float64)
    if np.isnan(y).any():
        raise ValueError("Input y contains NaN.")
    if np.isinf(y).any():
        raise ValueError("Input y contains infinity or a value too large for dtype('float64').")


def _splitter_of(kind):
    if kind in _TREE_SPLITTERS:
        return kind
    if kind not in _FOREST_FIT_KINDS:
        raise ValueError("tree ensemble %r: 'randomforest' or 'extratrees' (splitters 'best' / 'random')" % (kind,))
    return _FOREST_FIT_KINDS[kind]


def forest_tree_seeds(random_state, n_estimators):
    """Per tree the random_state a scikit-learn forest gives its estimators: check_random_state(random_state), then ONE
    randint(np.iinfo(np.int32).max) per tree, in order (None: NumPy's global state, an int: a fresh RandomState)."""
    if random_state is None:
        rs = np.random.mtrand._rand
    elif isinstance(random_state, np.random.RandomState):
        rs = random_state
    else:
        rs = _TREE_RS
        rs.seed(random_state)
    return [int(v) for v in rs.randint(np.iinfo(np.int32).max, size=int(n_estimators))] if int(n_estimators) > 0 else []


def tree_inputs(seed, n_rows, bootstrap):
    """What NumPy draws for ONE tree of a forest whose estimator has random_state=seed: (the splitter's rand_r seed,
    RandomState(seed).randint(0, RAND_R_MAX); the in-bag counts of a bootstrap, np.bincount of
    RandomState(seed).randint(0, n, n, dtype=np.int32), or None).  Both are first draws of their own RandomState(seed)."""
    _TREE_RS.seed(seed)                           # re-seeding one RandomState gives RandomState(seed)'s stream at a twentieth of the cost
    rand_r = int(_TREE_RS.randint(0, RAND_R_MAX))
    if not bootstrap:
        return rand_r, None
    _TREE_RS.seed(seed)
    picks = _TREE_RS.randint(0, n_rows, n_rows, dtype=np.int32)
    return rand_r, np.bincount(picks, minlength=n_rows).astype(np.int32)


class TreeFitResult:
    """What tree_fit returns: trees, one dict per task with scikit-learn's tree_ arrays (children_left, children_right, feature,
    threshold, impurity, n_node_samples, weighted_n_node_samples, missing_go_to_left, value [nodes][n_classes]), and classes, per
    task the classes present among its rows, ascending."""

    def __init__(self, trees, classes):
        self.trees, self.classes = trees, classes


def tree_fit(X, tasks, splitter):
    """Decision trees over ONE sample matrix, all built side by side (paa_tree_fit_tasks_f64, tree_fit_kernel: scikit-learn
    1.7.2's DepthFirstTreeBuilder with Gini, max_features='sqrt', no depth limit, bit for bit).  X [n_samples][n_dims]; a task is
    (rows, y, weights, seed, mean, scale): the rows X[rows] standardised as float32((x - mean) / scale), their labels y
    (re-encoded to the classes present, as np.unique does), integer weights (0: out of the bag; None: all 1) and the
    splitter's rand_r seed.  splitter: 'best' (DecisionTreeClassifier, 'randomforest') or 'random' (ExtraTreeClassifier,
    'extratrees').  Tasks that pass the SAME rows, y, mean and scale objects share one float32 copy on the device.  More than
    8192 rows in a task raise NotImplementedError, NaN / infinity scikit-learn's ValueError.  Returns a TreeFitResult."""
    return _tree_fit(X, tasks, _splitter_of(splitter))


def tree_fit_regression(X, tasks):
    """Regression trees over ONE sample matrix, all built side by side (paa_tree_fit_reg_tasks_f64, the squared-error instance of
    tree_fit_kernel: scikit-learn 1.7.2's DecisionTreeRegressor as a RandomForestRegressor fits it -- best splitter, every feature,
    no depth limit).  X and the tasks (rows, y, weights, seed, mean, scale) are tree_fit's, y being float targets.  The kernel forms
    every floating-point sum in a fixed order, so a tree is bit-identical run to run, alone or in any batch; when targets and weights
    make the sums exact in FP64 (e.g. multiples of 1/8 within +-1024 and a total weight <= 8192) every array equals scikit-learn's bit
    for bit, otherwise it is a valid CART tree whose sums may differ from scikit-learn's in the last places.
    NaN / infinity in y raise scikit-learn's ValueError and more than 8192 rows NotImplementedError, before the library is asked.
    Returns a TreeFitResult with value [nodes][1] and classes None."""
    return _tree_fit(X, tasks, None)


def tree_fit_boosting(X, tasks, max_depth=3):
    """The regression trees of gradient-boosting stages over ONE sample matrix, all built side by side (paa_tree_fit_boost_tasks_f64,
    the Friedman instance of tree_fit_kernel: scikit-learn 1.7.2's DecisionTreeRegressor(criterion="friedman_mse", max_depth) -- best
    splitter, every feature, a node at max_depth is a leaf).  X and the tasks (rows, y, weights, seed, mean, scale) are
    tree_fit_regression's, and so are the fixed summation order, the exactness rule (targets that are multiples of 1/8 within +-1024
    give scikit-learn's arrays bit for bit), the refusals and the result: value [nodes][1] holds the node means (no leaf step)."""
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or max_depth < 1:
        raise ValueError("max_depth = %r: an integer >= 1" % (max_depth,))
    return _tree_fit(X, tasks, None, int(max_depth))


def _tree_fit(X, tasks, splitter, max_depth=None):
    """tree_fit (splitter 'best' / 'random'), tree_fit_regression (splitter None) and tree_fit_boosting (... with max_depth)."""
    regression = splitter is None
    X = np.ascontiguousarray(X, dtype=np.float64)
    tasks = list(tasks)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("sample matrix of shape %s" % (X.shape,))
    if not tasks:
        raise ValueError("no tasks")
    n_samples, n_dims = X.shape
    job_of, rows_l, label_l, k_l, means, scales, classes_l = {}, [], [], [], [], [], []
    task_job, seeds, weights = [], [], []
    for t, task in enumerate(tasks):
        if len(task) != 6:
            raise ValueError("task %d: (rows, y, weights, seed, mean, scale) expected" % t)
        key = tuple(id(task[i]) for i in (0, 1, 4, 5))
        if key not in job_of:
            r = _index_list(task[0], "row", t)
            y = np.asarray(task[1]).reshape(-1)
            if y.shape[0] != r.shape[0]:
                raise ValueError("task %d: %d rows and %d labels" % (t, r.shape[0], y.shape[0]))
            _check_tree_rows(r.shape[0], "task %d" % t)
            mean, scale = _stats(task[4], task[5], n_dims)
            if regression:
                _check_targets(y)
                classes, idx = None, np.asarray(y, dtype=np.float64)
            else:
                classes, idx = np.unique(y, return_inverse=True) if y.shape[0] else (y, y)
            job_of[key] = len(rows_l)
            rows_l.append(r)
            label_l.append(idx.astype(np.float64 if regression else np.int32).reshape(-1))
            k_l.append(1 if regression else int(classes.shape[0]))
            classes_l.append(classes)
            means.append(mean)
            scales.append(scale)
        j = job_of[key]
        n = rows_l[j].shape[0]
        w = np.ones(n, dtype=np.int64) if task[2] is None else np.asarray(task[2]).reshape(-1)
        if w.shape[0] != n or (w.size and w.dtype.kind not in "iub"):
            raise ValueError("task %d: %d rows and weights of shape %s, dtype %s (integers expected)" % (t, n, w.shape, w.dtype))
        task_job.append(j)
        seeds.append(int(task[3]))
        weights.append(np.clip(w.astype(np.int64), -1, TREE_MAX_WEIGHT + 1).astype(np.int32))
    idx, off = _packed(rows_l, np.int32)
    label = np.ascontiguousarray(np.concatenate(label_l), dtype=np.float64 if regression else np.int32)
    k = np.array(k_l, dtype=np.int32)
    mean, scale = np.stack(means), np.stack(scales)
    task_job = np.array(task_job, dtype=np.int32)
    seed = np.array(seeds, dtype=np.int64)
    weight = np.ascontiguousarray(np.concatenate(weights), dtype=np.int32)
    caps = np.array([max(2 * int(np.count_nonzero(w)) - 1, 0) for w in weights], dtype=np.int64)
    node_off = _offsets(caps)
    val_off = _offsets(caps * k[task_job])
    total_nodes, total_values, n_tasks = int(node_off[-1]), int(val_off[-1]), len(tasks)
    count, out, pointers = _tree_outputs(n_tasks, total_nodes, total_values)
    value = out.pop("value")
    flags = np.zeros(len(rows_l), dtype=np.int32)
    head = (_ffi.as_f64p(X), n_samples, n_dims, len(rows_l), _ffi.as_i64p(off), _ffi.as_i32p(idx))
    middle = (_ffi.as_f64p(mean), _ffi.as_f64p(scale), n_tasks, _ffi.as_i32p(task_job), _ffi.as_i64p(seed), _ffi.as_i32p(weight))
    tail = (total_nodes, total_values, _ffi.as_i32p(flags)) + pointers
    if regression and max_depth is not None:
        _ffi.check(_ffi.lib().paa_tree_fit_boost_tasks_f64(*head, _ffi.as_f64p(label), *middle, max_depth, *tail))
    elif regression:
        _ffi.check(_ffi.lib().paa_tree_fit_reg_tasks_f64(*head, _ffi.as_f64p(label), *middle, *tail))
    else:
        _ffi.check(_ffi.lib().paa_tree_fit_tasks_f64(*head, _ffi.as_i32p(label), _ffi.as_i32p(k), *middle, _TREE_SPLITTERS[splitter], *tail))
    _raise_tree_flags(flags)
    trees = []
    for t in range(n_tasks):
        a, n_nodes, kt = int(node_off[t]), int(count[t]), int(k[task_job[t]])
        tree = {name: arr[a:a + n_nodes].astype(np.int64) if arr.dtype == np.int32 else arr[a:a + n_nodes].copy() for name, arr in out.items()}
        tree["value"] = value[int(val_off[t]):int(val_off[t]) + n_nodes * kt].reshape(n_nodes, kt).copy()
        trees.append(tree)
    return TreeFitResult(trees, None if regression else [classes_l[j] for j in task_job])


class _ClassSplitResult(_SplitResult):
    def job(self, j):
        """(labels, probabilities [n_test][classes present in job j] or None) of job j."""
        r = self._rows(j)
        return self.label[r], None if self.proba is None else self.proba[r, :len(self.classes[j])]


class ForestSplitResult(_ClassSplitResult):
    """What forest_split_fit_predict returns: label [Q] (class values as in `labels`), proba [Q][max_classes] or None (column c:
    the job's c-th present class; zeros past a job's classes), test_off [n_jobs + 1], classes (per job the classes present in its
    training list, ascending), n_estimators [n_jobs] and the number of chunks the trees were fitted in."""

    def __init__(self, label, proba, test_off, classes, n_estimators, n_chunks):
        self.label, self.proba, self.test_off, self.classes, self.n_estimators, self.n_chunks = label, proba, test_off, classes, n_estimators, n_chunks


_TreeSweep = collections.namedtuple("_TreeSweep", "counts n_est head flags chunks")


def _tree_sweep(p, y_pointer):
    """The shared opening of a tree sweep over the packed jobs p: every training list is checked against TREE_MAX_ROWS; counts (rows
    per training list), n_est [n_jobs], head (the arguments X .. n_estimators of the library call, y_pointer as the labels or
    targets) and the flags [n_jobs] and chunks [1] the call writes."""
    n_jobs = len(p.last)
    counts = np.diff(p.train_off)
    for j in range(n_jobs):
        _check_tree_rows(int(counts[j]), "job %d" % j)
    n_est = np.array([max(v[0], 0) for v in p.last], dtype=np.int32)
    head = (_ffi.as_f64p(p.X), p.X.shape[0], p.X.shape[1], y_pointer, n_jobs, _ffi.as_i64p(p.train_off), _ffi.as_i32p(p.train_idx),
            _ffi.as_i64p(p.test_off), _ffi.as_i32p(p.test_idx), _ffi.as_f64p(p.mean), _ffi.as_f64p(p.scale), _ffi.as_i32p(n_est))
    return _TreeSweep(counts, n_est, head, np.zeros(n_jobs, dtype=np.int32), np.zeros(1, dtype=np.int32))


def _forest_sweep(p, y_pointer, bootstrap):
    """_tree_sweep and what NumPy draws for the forests of the jobs: per job forest_tree_seeds(seed, n_estimators), per tree
    tree_inputs (bootstrap: with the in-bag counts).  Returns (the _TreeSweep, the (seed, weight) arguments of the library call)."""
    sw = _tree_sweep(p, y_pointer)
    seeds, weights = [], []
    for j in range(len(p.last)):
        for s in forest_tree_seeds(p.last[j][1], sw.n_est[j]):
            rand_r, w = tree_inputs(s, int(sw.counts[j]), bootstrap and sw.counts[j] > 0)
            seeds.append(rand_r)
            if w is not None:
                weights.append(w)
    seed = np.array(seeds, dtype=np.int64)
    weight = np.ascontiguousarray(np.concatenate(weights), dtype=np.int32) if weights else None
    return sw, (_ffi.as_i64p(seed), _ffi.as_i32p(weight) if weight is not None else None)


def forest_split_fit_predict(X, labels, jobs, kind, proba=False):
    """RandomForestClassifier / ExtraTreesClassifier(n_estimators, random_state=seed).fit(train).predict(test) for every job of a
    sweep over ONE sample matrix (paa_forest_fit_splits_f64: one workgroup per tree, the trees of all jobs side by side in chunks of
    bounded device scratch; every test row is scored on the device by the traversal and reduction kernels of forest_predict, no
    tree crosses to the host).  X [n_samples][n_dims]; labels [n_samples] (integers >= 0 on the training rows); a job is
    (train_idx, test_idx, mean, scale, (n_estimators, seed)); kind 'randomforest' (bootstrap) or 'extratrees'.  The host does what
    NumPy does for scikit-learn: per job forest_tree_seeds(seed, n_estimators), per tree tree_inputs.  Labels and probabilities
    equal scikit-learn's for the same seeds bit for bit.  A training list above 8192 rows raises NotImplementedError before the
    device is touched; NaN / infinity raise scikit-learn's ValueError.  Returns a ForestSplitResult."""
    if kind not in _FOREST_FIT_KINDS:
        raise ValueError("tree ensemble %r: 'randomforest' or 'extratrees'" % (kind,))
    p = _pack_jobs(X, labels, jobs, "(n_estimators, seed)", lambda v: (int(v[0]), v[1]))
    sw, drawn = _forest_sweep(p, _ffi.as_i32p(p.labels), kind == "randomforest")
    classes = [np.unique(p.labels[rows]) for rows in p.inside]
    Q, max_classes = int(p.test_off[-1]), max(max(len(c) for c in classes), 1)
    label = np.zeros(Q, dtype=np.int32)
    P = np.zeros((Q, max_classes), dtype=np.float64) if proba else None
    _ffi.check(_ffi.lib().paa_forest_fit_splits_f64(
        *sw.head, _TREE_SPLITTERS[_FOREST_FIT_KINDS[kind]], *drawn, _ffi.as_i32p(label), _ffi.as_f64p(P) if proba else None, max_classes,
        _ffi.as_i32p(sw.flags), _ffi.as_i32p(sw.chunks)))
    _raise_tree_flags(sw.flags)
    ForestModel._raise_invalid(label)
    return ForestSplitResult(label.astype(np.int64), P, p.test_off, classes, sw.n_est, int(sw.chunks[0]))


def _device_fit_inputs(features, labels, n_estimators, random_state=None, bootstrap=None, regression=False):
    """The shared opening of the train_*_device functions: the checks of the sample matrix, the labels (regression: float targets,
    validated as scikit-learn does), n_estimators and the row limit; rows, mean and scale of the one job over all rows; the
    tree_fit tasks of a forest, drawn as scikit-learn draws them (bootstrap None: no forest, nothing is drawn).  Returns (X, y,
    rows, mean, scale, tasks)."""
    X = np.ascontiguousarray(features, dtype=np.float64)
    y = np.asarray(labels, dtype=np.float64 if regression else None).reshape(-1)
    if X.ndim != 2 or X.shape[0] < 1 or y.shape[0] != X.shape[0]:
        raise ValueError("sample matrix of shape %s with %d %s" % (X.shape, y.shape[0], "targets" if regression else "labels"))
    if int(n_estimators) < 1:
        raise ValueError("n_estimators = %r" % (n_estimators,))
    if regression:
        _check_targets(y)
    n, n_dims = X.shape
    _check_tree_rows(n, "the training set")
    rows, mean, scale = np.arange(n), np.zeros(n_dims), np.ones(n_dims)
    tasks = []
    for s in forest_tree_seeds(random_state, n_estimators) if bootstrap is not None else ():
        rand_r, w = tree_inputs(s, n, bootstrap)
        tasks.append((rows, y, w, rand_r, mean, scale))
    return X, y, rows, mean, scale, tasks


def _forest_of_trees(kind, trees, classes, n_dims):
    """The ForestArrays of kind "averaged" / "regressor" of tree_fit's trees, with impurity, n_node_samples and
    weighted_n_node_samples beside them."""
    cat = lambda name: np.concatenate([t[name] for t in trees])        # noqa: E731
    arrays = ForestArrays(kind, _offsets([t["feature"].shape[0] for t in trees]), cat("children_left"), cat("children_right"), cat("feature"),
                          cat("threshold"), cat("missing_go_to_left"), cat("value") if kind == "averaged" else cat("value")[:, 0], classes, n_dims)
    arrays.impurity, arrays.n_node_samples, arrays.weighted_n_node_samples = cat("impurity"), cat("n_node_samples"), cat("weighted_n_node_samples")
    return arrays


def train_forest_device(features, labels, n_estimators, kind="randomforest", *, random_state=None):
    """train_random_forest / train_extra_trees on the GPU: RandomForestClassifier / ExtraTreesClassifier(n_estimators,
    random_state=random_state).fit(features, labels) by tree_fit -- per tree the seed scikit-learn's forest draws
    (forest_tree_seeds; None: from NumPy's global state exactly as scikit-learn does), the splitter's rand_r seed and, for
    'randomforest', the bootstrap counts (tree_inputs).  Returns a ForestArrays of kind "averaged" whose arrays equal those of
    scikit-learn's estimators_ bit for bit (it also carries impurity, n_node_samples and weighted_n_node_samples, for
    to_sklearn_forest), so forest_model, forest_predict, classifier_wrapper and device_model take it.  More than 8192 rows raise
    NotImplementedError before the device is touched; there is no CPU fallback."""
    if kind not in _FOREST_FIT_KINDS:
        raise ValueError("tree ensemble %r: 'randomforest' or 'extratrees'" % (kind,))
    X, _, _, _, _, tasks = _device_fit_inputs(features, labels, n_estimators, random_state, kind == "randomforest")
    res = tree_fit(X, tasks, kind)
    return _forest_of_trees("averaged", res.trees, res.classes[0], X.shape[1])


def _tree_depth(left, right):
    """The depth of a tree given by its children arrays, level by level."""
    depth, level = 0, np.zeros(1, dtype=np.int64)
    while True:
        below = np.concatenate([left[level], right[level]])
        level = below[below >= 0]
        if not level.size:
            return depth
        depth += 1


def _sklearn_tree(a, lo, hi, n_outputs_of_value, value):
    """The sklearn.tree._tree.Tree (built through __setstate__) of the nodes lo .. hi - 1 of the ForestArrays a, whose values are
    value[lo:hi] with n_outputs_of_value columns; impurity, n_node_samples and weighted_n_node_samples where a carries them."""
    from sklearn.tree._tree import NODE_DTYPE, Tree
    nodes = np.zeros(hi - lo, dtype=NODE_DTYPE)
    nodes["left_child"], nodes["right_child"] = a.children_left[lo:hi], a.children_right[lo:hi]
    nodes["feature"], nodes["threshold"] = a.feature[lo:hi], a.threshold[lo:hi]
    nodes["missing_go_to_left"] = a.missing_go_to_left[lo:hi]
    for name in ("impurity", "n_node_samples", "weighted_n_node_samples"):
        if getattr(a, name, None) is not None:
            nodes[name] = getattr(a, name)[lo:hi]
    tree = Tree(a.n_dims, np.array([n_outputs_of_value], dtype=np.intp), 1)
    tree.__setstate__({"max_depth": _tree_depth(nodes["left_child"], nodes["right_child"]), "node_count": hi - lo, "nodes": nodes,
                       "values": np.ascontiguousarray(value[lo:hi].reshape(hi - lo, 1, n_outputs_of_value))})
    return tree


def to_sklearn_forest(arrays, kind):
    """A real fitted sklearn.ensemble.RandomForestClassifier ('randomforest') / ExtraTreesClassifier ('extratrees') with the trees of
    a ForestArrays of kind "averaged" (every Tree is built through __setstate__): it predicts as scikit-learn predicts from those
    arrays and pickles as the reference's model files do.  impurity, n_node_samples and weighted_n_node_samples are those of
    train_forest_device when the arrays carry them, zeros otherwise (prediction reads none of them).  Needs scikit-learn."""
    import sklearn.ensemble
    if kind not in _FOREST_FIT_KINDS:
        raise ValueError("tree ensemble %r: 'randomforest' or 'extratrees'" % (kind,))
    a = forest_arrays(arrays)
    if a.kind != "averaged":
        raise ValueError("a tree ensemble of kind %r: 'averaged' expected" % (a.kind,))
    n_trees, k = a.node_offsets.shape[0] - 1, a.n_classes
    cls = sklearn.ensemble.RandomForestClassifier if kind == "randomforest" else sklearn.ensemble.ExtraTreesClassifier
    forest = cls(n_estimators=n_trees)
    forest._validate_estimator()
    forest.classes_ = np.asarray(a.classes_)
    forest.n_classes_ = k
    forest.n_features_in_ = a.n_dims
    forest.n_outputs_ = 1
    value = a.value.reshape(-1, k)
    forest.estimators_ = []
    for t in range(n_trees):
        tree = _sklearn_tree(a, int(a.node_offsets[t]), int(a.node_offsets[t + 1]), k, value)
        est = forest._make_estimator(append=False)
        est.tree_ = tree
        est.classes_, est.n_classes_ = forest.classes_, k
        est.n_features_in_, est.n_outputs_, est.max_features_ = a.n_dims, 1, max(1, int(np.sqrt(a.n_dims)))
        forest.estimators_.append(est)
    return forest


class ForestRegressionSplitResult(_SplitResult):
    """What forest_regression_split_fit_predict returns: pred [Q] (the test predictions), train_pred [T] or None (the predictions of
    every job's own training rows, job j owns train_off[j] .. train_off[j + 1] - 1), test_off / train_off [n_jobs + 1],
    n_estimators [n_jobs] and the number of chunks the trees were fitted in."""

    def __init__(self, pred, train_pred, test_off, train_off, n_estimators, n_chunks):
        self.pred, self.train_pred, self.test_off, self.train_off = pred, train_pred, test_off, train_off
        self.n_estimators, self.n_chunks = n_estimators, n_chunks

    def job(self, j):
        """(test predictions, training predictions or None) of job j."""
        t0, t1 = int(self.train_off[j]), int(self.train_off[j + 1])
        return self.pred[self._rows(j)], None if self.train_pred is None else self.train_pred[t0:t1]


def forest_regression_split_fit_predict(X, y, jobs, train_pred=False):
    """RandomForestRegressor(n_estimators, random_state=seed).fit(train).predict(test) for every job of a sweep over ONE sample
    matrix (paa_forest_reg_fit_splits_f64: one workgroup per tree, chunks of bounded device scratch, every test row -- with
    train_pred=True every job's training rows too -- scored on the device as the averaged forest with one output; no tree crosses to
    the host).  X [n_samples][n_dims]; y [n_samples] float targets; a job is (train_idx, test_idx, mean, scale, (n_estimators,
    seed)).  The host draws exactly what it draws for the classifier: per job forest_tree_seeds(seed, n_estimators), per tree
    tree_inputs(..., bootstrap=True).  Predictions equal scikit-learn's bit for bit when the targets make the trees' sums exact (see
    tree_fit_regression); otherwise they are those of valid CART trees.  NaN / infinity in y raise scikit-learn's ValueError and a
    training list above 8192 rows NotImplementedError, before the library is asked.  Returns a ForestRegressionSplitResult."""
    p = _pack_jobs(X, y, jobs, "(n_estimators, seed)", lambda v: (int(v[0]), v[1]))
    targets = _targets(p.raw, p.X.shape[0])
    _check_targets(targets)
    sw, drawn = _forest_sweep(p, _ffi.as_f64p(targets), True)
    Q, T = int(p.test_off[-1]), int(p.train_off[-1])
    pred = np.zeros(Q)
    tp = np.zeros(T) if train_pred else None
    _ffi.check(_ffi.lib().paa_forest_reg_fit_splits_f64(*sw.head, *drawn, _ffi.as_f64p(pred), _ffi.as_f64p(tp) if train_pred else None,
                                                        _ffi.as_i32p(sw.flags), _ffi.as_i32p(sw.chunks)))
    _raise_tree_flags(sw.flags)
    return ForestRegressionSplitResult(pred, tp, p.test_off, p.train_off, sw.n_est, int(sw.chunks[0]))


def train_random_forest_regression_device(features, labels, n_estimators, *, random_state=None):
    """train_random_forest_regression on the GPU: RandomForestRegressor(n_estimators, random_state=random_state).fit(features,
    labels) by tree_fit_regression -- per tree the seed scikit-learn's forest draws (forest_tree_seeds; None: from NumPy's global
    state exactly as scikit-learn does), the splitter's rand_r seed and the bootstrap counts (tree_inputs).  Returns (a ForestArrays
    of kind "regressor", which forest_model, regress and regression_wrapper take and which carries impurity, n_node_samples and
    weighted_n_node_samples for to_sklearn_forest_regressor; the mean absolute training error, from the device prediction).  The
    arrays equal those of scikit-learn's estimators_ bit for bit when the targets make the trees' sums exact (tree_fit_regression).
    More than 8192 rows raise NotImplementedError before the device is touched; there is no CPU fallback."""
    X, y, _, mean, scale, tasks = _device_fit_inputs(features, labels, n_estimators, random_state, True, regression=True)
    arrays = _forest_of_trees("regressor", tree_fit_regression(X, tasks).trees, None, X.shape[1])
    pred = regress([arrays], "randomforest", X.T, mean, scale)[0]
    return arrays, np.mean(np.abs(pred - y))


def to_sklearn_forest_regressor(arrays):
    """A real fitted sklearn.ensemble.RandomForestRegressor with the trees of a ForestArrays of kind "regressor" (every Tree is built
    through __setstate__): it predicts as scikit-learn predicts from those arrays and pickles as the reference's regression model
    files do.  impurity, n_node_samples and weighted_n_node_samples are those of train_random_forest_regression_device when the
    arrays carry them, zeros otherwise (prediction reads none of them).  Needs scikit-learn."""
    import sklearn.ensemble
    a = forest_arrays(arrays)
    if a.kind != "regressor":
        raise ValueError("a tree ensemble of kind %r: 'regressor' expected" % (a.kind,))
    n_trees = a.node_offsets.shape[0] - 1
    forest = sklearn.ensemble.RandomForestRegressor(n_estimators=n_trees)
    forest._validate_estimator()
    forest.n_features_in_ = a.n_dims
    forest.n_outputs_ = 1
    value = a.value.reshape(-1)
    forest.estimators_ = []
    for t in range(n_trees):
        tree = _sklearn_tree(a, int(a.node_offsets[t]), int(a.node_offsets[t + 1]), 1, value)
        est = forest._make_estimator(append=False)
        est.tree_ = tree
        est.n_features_in_, est.n_outputs_, est.max_features_ = a.n_dims, 1, a.n_dims
        forest.estimators_.append(est)
    return forest


BOOST_LEARNING_RATE, BOOST_MAX_DEPTH = 0.1, 3    # GradientBoostingClassifier's defaults, which train_gradient_boosting keeps


def boosting_tree_seeds(random_state, n_trees):
    """Per tree of a GradientBoostingClassifier the rand_r seed of its splitter: scikit-learn hands every tree of the ensemble the SAME
    RandomState (check_random_state(random_state): None is NumPy's global state, an int a fresh RandomState), and every tree's
    splitter draws ONE randint(0, RAND_R_MAX) from it, stage after stage and within a stage class after class."""
    if random_state is None:
        rs = np.random.mtrand._rand
    elif isinstance(random_state, np.random.RandomState):
        rs = random_state
    else:
        rs = _TREE_RS
        rs.seed(random_state)
    return [int(v) for v in rs.randint(0, RAND_R_MAX, size=int(n_trees))] if int(n_trees) > 0 else []


def boosting_init(class_index, n_classes):
    """The constant initial raw score of a GradientBoostingClassifier (init=None) on rows with the class indices class_index in
    0 .. n_classes - 1: DummyClassifier(strategy="prior")'s class fractions, clipped to float32's eps, through the loss's link --
    scikit-learn's own link objects, so the bits are its bits (8 balanced classes give -2.2e-16, not 0).  [1] for two classes."""
    from sklearn._loss.link import LogitLink, MultinomialLogit
    counts = np.bincount(np.asarray(class_index, dtype=np.int64), minlength=int(n_classes))
    prior = counts / counts.sum()
    eps = np.finfo(np.float32).eps
    if n_classes == 2:
        return np.asarray(LogitLink().link(np.clip(prior[1:2], eps, 1 - eps, dtype=np.float64)), dtype=np.float64).reshape(1)
    return np.asarray(MultinomialLogit().link(np.clip(prior.reshape(1, -1), eps, 1 - eps, dtype=np.float64)), dtype=np.float64)[0]


def _boost_tree_cap(n, max_depth):
    return min(2 * n - 1, 2 ** (max_depth + 1) - 1)


class BoostingSplitResult(_ClassSplitResult):
    """What boosting_split_fit_predict returns: label [Q] (class values as in `labels`), proba [Q][max_classes] or None (column c: the
    job's c-th present class; zeros past a job's classes), test_off [n_jobs + 1], classes (per job the classes present in its training
    list, ascending), n_estimators [n_jobs], the number of chunks the jobs were fitted in and, with train_score=True, per job
    train_score (scikit-learn's train_score_ [n_estimators]), train_raw (the raw predictions of its training rows after the last
    stage, [n][n_outputs]) and train_resid (the negative gradients its last stage's trees were fitted to, [n][n_outputs]), else None; models: per job a ForestArrays of kind "boosted" when the trees were asked for, else None."""

    def __init__(self, label, proba, test_off, classes, n_estimators, n_chunks, train_score, train_raw, train_resid, models):
        self.label, self.proba, self.test_off, self.classes, self.n_estimators, self.n_chunks = label, proba, test_off, classes, n_estimators, n_chunks
        self.train_score, self.train_raw, self.train_resid, self.models = train_score, train_raw, train_resid, models


def boosting_split_fit_predict(X, labels, jobs, proba=False, train_score=False, *, trees=False, chunk_bytes=None):
    """GradientBoostingClassifier(n_estimators, random_state=seed).fit(train).predict(test) for every job of a sweep over ONE sample
    matrix (paa_boost_fit_splits_f64: per stage one gradient launch and one tree launch over all jobs that still have stages, one
    workgroup per (job, class) tree, which also takes the leaves' Newton steps and updates the raw predictions; every test row is
    scored on the device by the boosted path of forest_predict; no tree crosses to the host unless trees=True).  X [n_samples][n_dims];
    labels [n_samples] (integers >= 0 on the training rows); a job is (train_idx, test_idx, mean, scale, (n_estimators, seed)).  The
    host does what NumPy does for scikit-learn: per job boosting_tree_seeds(seed, stages x trees per stage) and boosting_init.  A
    model is a function of its job alone (bit-identical alone, in any batch and chunking); stage 0 of a balanced job with 2, 4 or 8
    classes equals scikit-learn's bit for bit, later stages are those of a valid boosted model whose sums may differ from
    scikit-learn's in the last places.  A training list above 8192 rows raises NotImplementedError and one
    that holds a single class scikit-learn's ValueError, before the library is asked; NaN / infinity raise scikit-learn's ValueError.
    chunk_bytes (keyword only): a bound below the library's 1 GiB for the device scratch of one chunk of jobs (tests).  Returns a
    BoostingSplitResult."""
    p = _pack_jobs(X, labels, jobs, "(n_estimators, seed)", lambda v: (int(v[0]), v[1]))
    sw = _tree_sweep(p, _ffi.as_i32p(p.labels))
    n_dims, n_jobs, counts, n_est = p.X.shape[1], len(p.last), sw.counts, sw.n_est
    classes = [np.unique(p.labels[rows]) for rows in p.inside]
    for j in range(n_jobs):
        if counts[j] > 0 and len(classes[j]) < 2:
            raise ValueError("y contains %d class after sample_weight trimmed classes with zero weights, while a minimum of 2 classes "
                             "are required." % len(classes[j]))
    k_out = [1 if len(c) == 2 else len(c) for c in classes]
    max_classes = max(max(len(c) for c in classes), 2)
    init = np.zeros((n_jobs, max_classes), dtype=np.float64)
    seeds = []
    for j in range(n_jobs):
        seeds += boosting_tree_seeds(p.last[j][1], int(n_est[j]) * k_out[j])
        if len(classes[j]) >= 2:
            init[j, :k_out[j]] = boosting_init(np.searchsorted(classes[j], p.labels[p.inside[j]]), len(classes[j]))
    seed = np.array(seeds if seeds else [0], dtype=np.int64)
    Q, T = int(p.test_off[-1]), int(p.train_off[-1])
    label = np.zeros(Q, dtype=np.int32)
    P = np.zeros((Q, max_classes), dtype=np.float64) if proba else None
    score_off = _offsets(n_est)
    raw_off = _offsets([int(counts[j]) * k_out[j] for j in range(n_jobs)])
    score = np.zeros(max(int(score_off[-1]), 1)) if train_score else None
    raw = np.zeros(max(int(raw_off[-1]), 1)) if train_score else None
    resid = np.zeros(max(int(raw_off[-1]), 1)) if train_score else None
    caps = np.repeat([_boost_tree_cap(int(counts[j]), BOOST_MAX_DEPTH) for j in range(n_jobs)],
                     [int(n_est[j]) * k_out[j] for j in range(n_jobs)]).astype(np.int64) if trees else np.zeros(0, dtype=np.int64)
    node_off = _offsets(caps)
    total_nodes = int(node_off[-1]) if trees else 0
    count, out, pointers = _tree_outputs(len(caps), total_nodes, total_nodes)
    _ffi.check(_ffi.lib().paa_boost_fit_splits_f64(
        *sw.head, _ffi.as_i64p(seed), _ffi.as_f64p(init), max_classes, BOOST_LEARNING_RATE, BOOST_MAX_DEPTH, int(chunk_bytes or 0),
        _ffi.as_i32p(label), _ffi.as_f64p(P) if proba else None, _ffi.as_f64p(score) if train_score else None,
        _ffi.as_f64p(raw) if train_score else None, _ffi.as_f64p(resid) if train_score else None, total_nodes, *pointers,
        _ffi.as_i32p(sw.flags), _ffi.as_i32p(sw.chunks)))
    _raise_tree_flags(sw.flags)
    ForestModel._raise_invalid(label)
    scores = [score[int(score_off[j]):int(score_off[j + 1])].copy() for j in range(n_jobs)] if train_score else None
    raws = [raw[int(raw_off[j]):int(raw_off[j + 1])].reshape(int(counts[j]), k_out[j]).copy() for j in range(n_jobs)] if train_score else None
    resids = [resid[int(raw_off[j]):int(raw_off[j + 1])].reshape(int(counts[j]), k_out[j]).copy() for j in range(n_jobs)] if train_score else None
    models = None
    if trees:
        models, t0 = [], 0
        for j in range(n_jobs):
            n_trees = int(n_est[j]) * k_out[j]
            cut = lambda name: np.concatenate([out[name][int(node_off[t]):int(node_off[t]) + int(count[t])] for t in range(t0, t0 + n_trees)])   # noqa: E731
            m = ForestArrays("boosted", _offsets(count[t0:t0 + n_trees]), cut("children_left"), cut("children_right"), cut("feature"),
                             cut("threshold"), cut("missing_go_to_left"), cut("value"), classes[j], n_dims, BOOST_LEARNING_RATE, init[j, :k_out[j]])
            m.impurity, m.n_node_samples, m.weighted_n_node_samples = cut("impurity"), cut("n_node_samples").astype(np.int64), cut("weighted_n_node_samples")
            m.max_depth = BOOST_MAX_DEPTH
            cnt = np.bincount(np.searchsorted(classes[j], p.labels[p.inside[j]]), minlength=len(classes[j]))
            m.class_prior_ = cnt / cnt.sum()
            if train_score:
                m.train_score_ = scores[j]
            models.append(m)
            t0 += n_trees
    return BoostingSplitResult(label.astype(np.int64), P, p.test_off, classes, n_est, int(sw.chunks[0]), scores, raws, resids, models)


def train_gradient_boosting_device(features, labels, n_estimators, *, random_state=None):
    """train_gradient_boosting on the GPU: GradientBoostingClassifier(n_estimators, random_state=random_state).fit(features, labels)
    by boosting_split_fit_predict with one job over all rows (random_state None: the trees' seeds come from NumPy's global state
    exactly as scikit-learn draws them).  Returns a ForestArrays of kind "boosted", which forest_model, forest_predict,
    classifier_wrapper and device_model take, with train_score_ attached (and impurity, n_node_samples, weighted_n_node_samples for
    to_sklearn_boosting).  More than 8192 rows raise NotImplementedError and a single class scikit-learn's ValueError before the
    device is touched; there is no CPU fallback."""
    X, raw, rows, mean, scale, _ = _device_fit_inputs(features, labels, n_estimators)
    classes, idx = np.unique(raw, return_inverse=True)
    job = (rows, np.zeros(0, dtype=np.int64), mean, scale, (int(n_estimators), random_state))
    res = boosting_split_fit_predict(X, idx.reshape(-1), [job], train_score=True, trees=True)
    model = res.models[0]
    model.classes_ = classes
    return model


def to_sklearn_boosting(arrays):
    """A real fitted sklearn.ensemble.GradientBoostingClassifier with the trees of a ForestArrays of kind "boosted" (every Tree is
    built through __setstate__): estimators_ [stages][trees per stage] of DecisionTreeRegressors, init_ (a DummyClassifier with the
    class priors that give the arrays' initial raw score), classes_, n_trees_per_iteration_ and train_score_ (the arrays' when they
    carry it, zeros otherwise).  It predicts as scikit-learn predicts from those arrays, pickles as the reference's model files do,
    and load_model / classifier_wrapper read it unchanged.  Needs scikit-learn."""
    import sklearn.ensemble
    from sklearn.dummy import DummyClassifier
    from sklearn.tree import DecisionTreeRegressor
    a = forest_arrays(arrays)
    if a.kind != "boosted":
        raise ValueError("a tree ensemble of kind %r: 'boosted' expected" % (a.kind,))
    n_trees, k, k_out = a.node_offsets.shape[0] - 1, a.n_classes, a.n_outputs
    if k < 2 or n_trees < 1 or n_trees % k_out or a.init is None or a.init.shape[0] != k_out:
        raise ValueError("boosted ensemble: %d trees for %d outputs of %d classes" % (n_trees, k_out, k))
    n_stages = n_trees // k_out
    max_depth = int(getattr(a, "max_depth", BOOST_MAX_DEPTH))
    gb = sklearn.ensemble.GradientBoostingClassifier(n_estimators=n_stages, learning_rate=a.learning_rate, max_depth=max_depth)
    gb.classes_ = np.asarray(a.classes_)
    gb.n_classes_ = k
    gb.n_features_in_ = a.n_dims
    gb.n_trees_per_iteration_ = k_out
    gb.n_estimators_ = n_stages
    gb.max_features_ = a.n_dims
    gb._loss = gb._get_loss(sample_weight=None)
    # the priors whose link is the initial raw score: the fit's own when the arrays carry them, else softmax / expit of the score
    # (the link's inverse); _raw_predict_init clips and links them
    if getattr(a, "class_prior_", None) is not None:
        prior = np.asarray(a.class_prior_, dtype=np.float64)
    elif k_out == 1:
        p1 = 1.0 / (1.0 + np.exp(-a.init[0]))
        prior = np.array([1.0 - p1, p1])
    else:
        e = np.exp(a.init - np.max(a.init))
        prior = e / e.sum()
    init = DummyClassifier(strategy="prior")
    init.classes_, init.n_classes_, init.class_prior_ = np.arange(k), k, prior
    init.n_outputs_, init.sparse_output_, init._strategy, init.n_features_in_ = 1, False, "prior", a.n_dims
    gb.init_ = init
    gb.train_score_ = np.asarray(getattr(a, "train_score_", np.zeros(n_stages)), dtype=np.float64)
    value = a.value.reshape(-1)
    gb.estimators_ = np.empty((n_stages, k_out), dtype=object)
    for t in range(n_trees):
        tree = _sklearn_tree(a, int(a.node_offsets[t]), int(a.node_offsets[t + 1]), 1, value)
        est = DecisionTreeRegressor(criterion="friedman_mse", max_depth=max_depth)
        est.tree_ = tree
        est.n_features_in_, est.n_outputs_, est.max_features_ = a.n_dims, 1, a.n_dims
        gb.estimators_[t // k_out, t % k_out] = est
    return gb


def _check_boosting_fit(boosting_fit, classifier_name):
    if boosting_fit not in ("sklearn", "device"):
        raise ValueError("boosting_fit=%r: 'sklearn' or 'device'" % (boosting_fit,))
    if boosting_fit == "device" and classifier_name != "gradientboosting":
        raise ValueError("boosting_fit='device' serves the classifier type 'gradientboosting', not %r" % (classifier_name,))


def _draw_split(n_samples, train_percentage):
    """One random split as (train indices, test indices): train_test_split over the sample indices consumes NumPy's
    global state exactly as the reference's train_test_split(X, y, ...) (:648-649) does, and X[train], X[test], y[test]
    are its arrays in its row order."""
    from sklearn.model_selection import train_test_split
    return train_test_split(np.arange(n_samples), test_size=1 - train_percentage)


def evaluate_classifier(features, class_names, classifier_name, params, parameter_mode, list_of_ids=None, n_exp=-1,
                        train_percentage=0.90, smote=False, *, svm_fit="sklearn", forest_fit="sklearn", boosting_fit="sklearn",
                        kernel_cache="none", cache_bytes=None):
    """Picks the classifier parameter with the best cross-validated accuracy (parameter_mode 0) or macro F1 (1)
    (reference :576-771): for every value, n_exp random splits (n_exp = -1: int(50000 / n_samples) + 1), each with its own
    StandardScaler; with list_of_ids the n_exp GroupShuffleSplit(train_size=.8) splits are drawn once and shared by every value.
    "knn": a kNN has no fit, and nothing but the splits draws from NumPy's global state, so ALL splits are drawn up front in
    the reference's order (parameter-major), a scaler is fitted per split on the host and ONE knn_split_predict launch
    classifies every test vector of the sweep against index lists over the one resident sample matrix.
    The five scikit-learn types: per (value, experiment) split -> scaler -> scikit-learn fit in the reference's order (the
    fits draw from the same global state); the test rows of each fitted model are scored by the device models in one
    launch per model (predict).  The fits dominate: the launch removes the per-vector predict loop and nothing else.
    Confusion matrices, the missing-class repair, precision / recall / F1 / accuracy, the printed table and the return value
    (params[first arg-max]) are the reference's, on the host.  smote=True raises NotImplementedError.
    svm_fit="device" (keyword only; "svm" / "svm_rbf", any other type raises ValueError): as for kNN, ALL splits are drawn up
    front in parameter-major order, a scaler is fitted per split on the host and ONE svm_split_fit_predict call fits every
    pair of classes of every split on the GPU (libsvm's solver, no Platt cross-validation: the sweep reads vote labels only)
    and classifies every test row.  The one visible difference to the default: scikit-learn's probabilistic fits draw a libsvm
    seed from NumPy's global state between the splits, the device mode consumes that state for the splits only, so for one seed
    the two modes see different splits.  svm_fit="sklearn" (the default) is the behaviour described above, untouched.
    kernel_cache / cache_bytes (keyword only, read under svm_fit="device"; anything but their defaults raises ValueError
    otherwise) are svm_split_fit_predict's: "gram" solves every split's pairs from the split's one resident kernel matrix, with
    the same predictions.
    forest_fit="device" (keyword only; "randomforest" / "extratrees", any other type raises ValueError before any work): the same
    path -- ALL splits are drawn up front in parameter-major order, then ONE seed per split is drawn from NumPy's global state in
    job order (np.random.randint(np.iinfo(np.int32).max)), and ONE forest_split_fit_predict call fits the n_estimators trees of
    every split on the GPU and classifies every test row there.  Every split's predictions are those of scikit-learn's forest
    with random_state=<that seed> on the same split, bit for bit.  The one visible difference to the default: scikit-learn's
    fits draw their tree seeds from the global state between the splits, so for one np.random.seed the two modes see different
    splits.  A split above 8192 training rows raises NotImplementedError.  forest_fit="sklearn" (the default): untouched.
    boosting_fit="device" (keyword only; "gradientboosting", any other type raises ValueError naming boosting_fit before any work):
    the same path once more -- ALL splits up front in parameter-major order, then ONE seed per split in job order
    (np.random.randint(np.iinfo(np.int32).max)), and ONE boosting_split_fit_predict call fits the n_estimators stages of every split
    on the GPU and classifies every test row there.  Every split's model is a valid boosted model of scikit-learn's kind for
    random_state=<that seed> (stage 0 of balanced 2-, 4- and 8-class splits bit for bit; see boosting_split_fit_predict).
    boosting_fit="sklearn" (the default): untouched."""
    return evaluate_classifier_full(features, class_names, classifier_name, params, parameter_mode, list_of_ids, n_exp,
                                    train_percentage, smote, svm_fit=svm_fit, forest_fit=forest_fit, boosting_fit=boosting_fit,
                                    kernel_cache=kernel_cache, cache_bytes=cache_bytes)[0]


def evaluate_classifier_full(features, class_names, classifier_name, params, parameter_mode, list_of_ids=None, n_exp=-1,
                             train_percentage=0.90, smote=False, *, svm_fit="sklearn", forest_fit="sklearn", boosting_fit="sklearn",
                             kernel_cache="none", cache_bytes=None):
    """evaluate_classifier, returning (the chosen parameter, the confusion matrix of every parameter value, the predictions
    [parameter][experiment] of every split's test rows)."""
    if svm_fit not in ("sklearn", "device"):
        raise ValueError("svm_fit=%r: 'sklearn' or 'device'" % (svm_fit,))
    if svm_fit == "device" and classifier_name not in _SVM_TYPES:
        raise ValueError("svm_fit='device' serves the classifier types %s, not %r" % (" and ".join(_SVM_TYPES), classifier_name))
    _svc_cache_mode(kernel_cache, cache_bytes, svm_fit == "device", "svm_fit")
    if forest_fit not in ("sklearn", "device"):
        raise ValueError("forest_fit=%r: 'sklearn' or 'device'" % (forest_fit,))
    if forest_fit == "device" and classifier_name not in _FOREST_FIT_KINDS:
        raise ValueError("forest_fit='device' serves the classifier types %s, not %r" % (" and ".join(_FOREST_FIT_KINDS), classifier_name))
    _check_boosting_fit(boosting_fit, classifier_name)
    if smote:
        raise NotImplementedError("smote=True: imbalanced-learn's SMOTE makes training rows that are no rows of the sample "
                                  "matrix; this package does not resample")
    if classifier_name not in _CLASSIFIER_TYPES:
        raise NotImplementedError("classifier %r: one of %s" % (classifier_name, ", ".join(_CLASSIFIER_TYPES)))
    import sklearn.metrics
    from sklearn.preprocessing import StandardScaler
    X, y = features_to_matrix(features)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 2 or len(class_names) != len(features):
        raise ValueError("%d feature matrices stacked to shape %s for %d class names" % (len(features), X.shape, len(class_names)))
    n_classes = len(features)
    n_samples_total = X.shape[0]
    if n_exp == -1:
        n_exp = int(50000 / n_samples_total) + 1
    if list_of_ids:
        from sklearn.model_selection import GroupShuffleSplit
        shared = [(tr, te) for tr, te in GroupShuffleSplit(n_splits=n_exp, train_size=.8).split(X, y, list_of_ids)]

    # splits (and, but for kNN, fits) in the reference's order; predictions [parameter][experiment]
    splits, predictions = [], []
    for C_param in params:
        splits.append([])
        predictions.append([])
        for e in range(n_exp):
            print("Param = {0:.5f} - classifier Evaluation Experiment {1:d} of {2:d}".format(C_param, e + 1, n_exp))
            train_idx, test_idx = shared[e] if list_of_ids else _draw_split(n_samples_total, train_percentage)
            scaler = StandardScaler().fit(X[train_idx])
            splits[-1].append((train_idx, test_idx, scaler.mean_, scaler.scale_))
            if classifier_name != "knn" and svm_fit != "device" and forest_fit != "device" and boosting_fit != "device":
                classifier = _train_classifier(scaler.transform(X[train_idx]), y[train_idx], classifier_name, C_param)
                predictions[-1].append(list(predict(classifier, classifier_name, X[test_idx].T, scaler.mean_, scaler.scale_)[0])
                                       if len(test_idx) else [])
    if classifier_name == "knn" or svm_fit == "device" or forest_fit == "device" or boosting_fit == "device":       # one sweep over every split
        knn, cast = classifier_name == "knn", int if classifier_name == "knn" else float
        if forest_fit == "device" or boosting_fit == "device":  # (n_estimators, the ensemble's seed): one draw per job, in job order
            cast = lambda v: (int(v), int(np.random.randint(np.iinfo(np.int32).max)))      # noqa: E731
        jobs = [(tr, te, mean, scale, cast(C_param)) for C_param, row in zip(params, splits) for tr, te, mean, scale in row]
        res = knn_split_predict(X, y, jobs) if knn else forest_split_fit_predict(X, y, jobs, classifier_name) if forest_fit == "device" else \
            boosting_split_fit_predict(X, y, jobs) if boosting_fit == "device" else \
            svm_split_fit_predict(X, y, jobs, kernel="rbf" if classifier_name == "svm_rbf" else "linear", kernel_cache=kernel_cache,
                                  cache_bytes=cache_bytes)
        as_label = (lambda v: v) if knn else y.dtype.type      # kNN: the result's int64 as it is
        predictions = [[[as_label(v) for v in res.job(i * n_exp + e)[0]] for e in range(n_exp)] for i in range(len(splits))]

    ac_all, f1_all, f1_std_all, pre_all, rec_all, f1_classes_all, cms_all = [], [], [], [], [], [], []
    y_flat = np.asarray(y).reshape(-1)
    for row, preds in zip(splits, predictions):
        cm = np.zeros((n_classes, n_classes))
        f1_per_exp = []
        for (train_idx, test_idx, _, _), y_pred in zip(row, preds):
            y_test = y[test_idx]
            cmt = sklearn.metrics.confusion_matrix(y_test, y_pred)
            f1_per_exp.append(sklearn.metrics.f1_score(y_test, y_pred, average='macro'))
            if cmt.size != cm.size:             # a class in neither the test labels nor the predictions: its row and column
                missing = set(y_flat).difference(set(y_test.tolist() + y_pred))
                missing = [int(c) for c in list(missing)]
                for c in missing:
                    cmt = np.insert(cmt, c, 0, axis=0)
                for c in missing:
                    cmt = np.insert(cmt, c, 0, axis=1)
            cm = cm + cmt
        cm = cm + 0.0000000010
        rec = np.array([cm[c, c] / np.sum(cm[c, :]) for c in range(cm.shape[0])])
        pre = np.array([cm[c, c] / np.sum(cm[:, c]) for c in range(cm.shape[0])])
        f1 = 2 * rec * pre / (rec + pre)
        pre_all.append(pre)
        rec_all.append(rec)
        f1_classes_all.append(f1)
        ac_all.append(np.sum(np.diagonal(cm)) / np.sum(cm))
        cms_all.append(cm)
        f1_all.append(np.mean(f1))
        f1_std_all.append(np.std(f1_per_exp))

    print("\t\t", end="")
    for i, c in enumerate(class_names):
        print("{0:s}\t\t".format(c) if i == len(class_names) - 1 else "{0:s}\t\t\t".format(c), end="")
    print("OVERALL")
    print("\tC" + "\tPRE\tREC\tf1" * len(class_names) + "\t{0:s}\t{1:s}".format("ACC", "f1"))
    best_ac_ind = np.argmax(ac_all)
    best_f1_ind = np.argmax(f1_all)
    for i in range(len(pre_all)):
        line = "\t{0:.3f}".format(params[i])
        for c in range(len(pre_all[i])):
            line += "\t{0:.1f}\t{1:.1f}\t{2:.1f}".format(100.0 * pre_all[i][c], 100.0 * rec_all[i][c], 100.0 * f1_classes_all[i][c])
        line += "\t{0:.1f}\t{1:.1f}".format(100.0 * ac_all[i], 100.0 * f1_all[i])
        if i == best_f1_ind:
            line += "\t best f1"
        if i == best_ac_ind:
            line += "\t best Acc"
        print(line)
    if parameter_mode == 0:
        print("Confusion Matrix:")
        print_confusion_matrix(cms_all[best_ac_ind], class_names)
        return params[best_ac_ind], cms_all, predictions
    elif parameter_mode == 1:
        print("Confusion Matrix:")
        print_confusion_matrix(cms_all[best_f1_ind], class_names)
        print(f"Best macro f1 {100 * f1_all[best_f1_ind]:.1f}")
        print(f"Best macro f1 std {100 * f1_std_all[best_f1_ind]:.1f}")
        return params[best_f1_ind], cms_all, predictions
    return None, cms_all, predictions


def extract_features_and_train(paths, mid_window, mid_step, short_window, short_step, classifier_type, model_name,
                               compute_beat=False, train_percentage=0.90, dict_of_ids=None, use_smote=False, *, svm_fit="sklearn",
                               final_fit="sklearn", forest_fit="sklearn", boosting_fit="sklearn", kernel_cache="none", cache_bytes=None):
    """Segment-based feature extraction of one folder per class, parameter tuning and training of a classifier (reference
    :236-361): features from multiple_directory_feature_extraction (GPU), rows with NaN / Inf dropped, the parameter from
    evaluate_classifier (macro F1, n_exp = -1), a StandardScaler over all rows, the final fit, and the model files in the
    reference's format -- "knn": eleven pickles in model_name (load_model_knn); otherwise the pickled classifier in model_name
    and model_name + "MEANS" (load_model).  use_smote=True raises NotImplementedError.  svm_fit (keyword only) goes to the tuning
    step, evaluate_classifier, and nowhere else.  final_fit (keyword only): "sklearn" (the default) fits the final model with
    scikit-learn; "device" ("svm" / "svm_rbf" only, any other type raises ValueError before any work) fits it with
    train_svm_device and writes the model file in the reference's format, a pickled sklearn.svm.SVC, through to_sklearn_svc --
    the MEANS file is the same.  forest_fit (keyword only): "device" ("randomforest" / "extratrees" only, any other type raises
    ValueError before any work) tunes n_estimators with evaluate_classifier(forest_fit="device") AND makes the final fit with
    train_forest_device; the model file is a pickled RandomForestClassifier / ExtraTreesClassifier made by to_sklearn_forest.
    boosting_fit (keyword only): "device" ("gradientboosting" only, any other type raises ValueError before any work) tunes
    n_estimators with evaluate_classifier(boosting_fit="device") AND makes the final fit with train_gradient_boosting_device; the model
    file is a pickled GradientBoostingClassifier made by to_sklearn_boosting.  kernel_cache / cache_bytes (keyword only, read under
    svm_fit="device" and final_fit="device"; anything but their defaults raises ValueError when neither is set) go to the tuning
    step under svm_fit="device" and to train_svm_device under final_fit="device": the model file has the same bytes."""
    _check_boosting_fit(boosting_fit, classifier_type)
    if forest_fit not in ("sklearn", "device") or (forest_fit == "device" and classifier_type not in _FOREST_FIT_KINDS):
        raise ValueError("forest_fit=%r with the classifier type %r" % (forest_fit, classifier_type))
    if svm_fit not in ("sklearn", "device") or (svm_fit == "device" and classifier_type not in _SVM_TYPES):
        raise ValueError("svm_fit=%r with the classifier type %r" % (svm_fit, classifier_type))
    if final_fit not in ("sklearn", "device") or (final_fit == "device" and classifier_type not in _SVM_TYPES):
        raise ValueError("final_fit=%r with the classifier type %r" % (final_fit, classifier_type))
    _svc_cache_mode(kernel_cache, cache_bytes, svm_fit == "device" or final_fit == "device", "svm_fit / final_fit")
    tune_cache = dict(kernel_cache=kernel_cache, cache_bytes=cache_bytes) if svm_fit == "device" else {}
    if use_smote:
        raise NotImplementedError("use_smote=True: this package does not resample (see evaluate_classifier)")
    from sklearn.preprocessing import StandardScaler
    features, class_names, file_names = aF.multiple_directory_feature_extraction(paths, mid_window, mid_step, short_window,
                                                                                 short_step, compute_beat=compute_beat)
    file_names = [name for names in file_names for name in names]
    list_of_ids = [dict_of_ids[name] for name in file_names] if dict_of_ids else None
    if len(features) == 0:
        print("trainSVM_feature ERROR: No data found in any input folder!")
        return
    for i, feat in enumerate(features):
        if len(feat) == 0:
            print("trainSVM_feature ERROR: " + paths[i] + " folder is empty or non-existing!")
            return
    if classifier_type in _SVM_TYPES:
        classifier_par = np.array([0.001, 0.01, 0.5, 1.0, 5.0, 10.0, 20.0])
    elif classifier_type == "knn":
        classifier_par = np.array([1, 3, 5, 7, 9, 11, 13, 15])
    elif classifier_type in _FOREST_TYPES:
        classifier_par = np.array([10, 25, 50, 100, 200, 500])
    else:
        raise NotImplementedError("classifier %r: one of %s" % (classifier_type, ", ".join(_CLASSIFIER_TYPES)))
    kept = []
    for feat in features:
        if feat.ndim == 1:                      # a class of one sample
            feat = feat.reshape((1, feat.shape[0]))
        rows = []
        for row in feat:
            if np.isnan(row).any() or np.isinf(row).any():
                print("NaN Found! Feature vector not used for training")
            else:
                rows.append(row.tolist())
        kept.append(np.array(rows))
    features = kept
    best_param = evaluate_classifier(features, class_names, classifier_type, classifier_par, 1, list_of_ids, n_exp=-1,
                                     train_percentage=train_percentage, smote=use_smote, svm_fit=svm_fit,
                                     forest_fit=forest_fit, boosting_fit=boosting_fit, **tune_cache)
    print("Selected params: {0:.5f}".format(best_param))
    features, labels = features_to_matrix(features)
    scaler = StandardScaler()
    features = scaler.fit_transform(features)
    mean = scaler.mean_.tolist()
    std = scaler.scale_.tolist()
    if classifier_type == "knn":
        save_parameters(model_name, features.tolist(), labels.tolist(), mean, std, class_names, best_param, mid_window, mid_step,
                        short_window, short_step, compute_beat)
    else:
        if final_fit == "device":
            classifier = to_sklearn_svc(train_svm_device(features, labels, best_param,
                                                         kernel="rbf" if classifier_type == "svm_rbf" else "linear",
                                                         kernel_cache=kernel_cache, cache_bytes=cache_bytes))
        elif forest_fit == "device":
            classifier = to_sklearn_forest(train_forest_device(features, labels, int(best_param), kind=classifier_type), classifier_type)
        elif boosting_fit == "device":
            classifier = to_sklearn_boosting(train_gradient_boosting_device(features, labels, int(best_param)))
        else:
            classifier = _train_classifier(features, labels, classifier_type, best_param)
        with open(model_name, "wb") as fid:
            cPickle.dump(classifier, fid)
        save_parameters(model_name + "MEANS", mean, std, class_names, mid_window, mid_step, short_window, short_step, compute_beat)


def _forest_regressor(model):
    fm = forest_model(model)
    if not fm.regressor:
        raise ValueError("a tree-ensemble classifier cannot regress")
    return fm


def regression_wrapper(model, model_type, test_sample):
    """The regression result of one feature vector (reference :96-111): "svm" / "svm_rbf" / "randomforest" give the
    model's predict() as a scalar, computed on the GPU; any other type gives None, as the reference falls through."""
    if model_type not in _REGRESSION_TYPES:
        return None
    x = np.asarray(test_sample, dtype=np.float64).reshape(-1, 1)
    return regress([model], model_type, x, np.zeros(x.shape[0]), np.ones(x.shape[0]))[0, 0]       # (x - 0) / 1 == x


def train_svm_regression(features, labels, c_param, kernel='linear'):
    """(fitted sklearn.svm.SVR, mean absolute training error) (reference :222-226): scikit-learn fits, the training
    error comes from the device prediction."""
    import sklearn.svm
    svm = sklearn.svm.SVR(C=c_param, kernel=kernel)
    svm.fit(features, labels)
    X = np.asarray(features, dtype=np.float64)
    pred = regress([svm], "svm", X.T, np.zeros(X.shape[1]), np.ones(X.shape[1]))[0]
    return svm, np.mean(np.abs(pred - labels))


def train_svm_regression_device(features, labels, c_param, kernel='linear', *, kernel_cache="gram"):
    """train_svm_regression on the GPU: SVR(C=c_param, kernel=kernel).fit(features, labels) as ONE task of svr_solve over all
    rows (mean 0, scale 1, epsilon 0.1, tol 1e-3; gamma 'scale' = 1 / (n_dims * features.var()), 1 when that variance is 0, as
    evaluate_regression's sweep forms it).  kernel_cache (keyword only) is svr_solve's, "gram" by default here: the one task
    is solved from its resident kernel matrix.  Returns (an SvrArrays-shaped model that also carries support_, dual_coef_,
    intercept_, C, epsilon, shape_fit_, n_features_in_ and fit_result, the mean absolute training error read from the
    solver's gradient).  More than 8192 rows raise NotImplementedError before the library is asked; there is no CPU
    fallback.  Agreement with scikit-learn is bounded by libsvm's stopping tolerance, not bit-exact."""
    kernel = _svr_kernel(kernel)
    X = np.ascontiguousarray(features, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("feature matrix of shape %s" % (X.shape,))
    if X.shape[0] > SMO_MAX_ROWS:
        raise NotImplementedError("%d training rows: the device solver serves at most %d per task" % (X.shape[0], SMO_MAX_ROWS))
    n, n_dims = X.shape
    y = _targets(labels, n)
    var = X.var()
    gamma = 1.0 / (n_dims * var) if kernel == "rbf" and var != 0 else 1.0
    res = svr_solve(X, y, [(np.arange(n), np.zeros(n_dims), np.ones(n_dims), float(c_param), gamma, 0.1)], kernel=kernel,
                    kernel_cache=kernel_cache)
    beta = res.beta[0]
    support = np.flatnonzero(beta != 0).astype(np.int32)
    model = SvrArrays(X[support], beta[support], [-res.rho[0]], gamma, kernel)
    model.support_ = support
    model.dual_coef_, model.intercept_ = model._dual_coef_, model._intercept_
    model.C, model.epsilon, model.shape_fit_, model.n_features_in_, model.fit_result = float(c_param), 0.1, X.shape, n_dims, res
    return model, np.mean(np.abs(res.train_pred[0] - y))


def to_sklearn_svr(model):
    """A real sklearn.svm.SVR with the fitted attributes of train_svm_regression_device's model, filled as to_sklearn_svc fills
    an SVC: it predicts as scikit-learn predicts from those arrays and pickles as the reference's model files do; regress,
    regression_wrapper, load_model(..., is_regression=True) and file_regression read it unchanged.  Needs scikit-learn."""
    import sklearn.svm
    svr = sklearn.svm.SVR(C=float(model.C), kernel=model.kernel, epsilon=float(model.epsilon))
    svr.support_ = np.asarray(model.support_, dtype=np.int32)
    svr.support_vectors_ = np.ascontiguousarray(model.support_vectors_, dtype=np.float64)
    svr._n_support = np.array([svr.support_.shape[0]] * 2, dtype=np.int32)     # as SVR.fit leaves it: the count, twice
    svr._dual_coef_ = np.ascontiguousarray(model._dual_coef_, dtype=np.float64).reshape(1, -1)
    svr._intercept_ = np.ascontiguousarray(model._intercept_, dtype=np.float64).reshape(-1)
    svr.dual_coef_ = svr._dual_coef_
    svr.intercept_ = svr._intercept_
    svr._probA = np.zeros(0)
    svr._probB = np.zeros(0)
    svr._gamma = float(model._gamma)
    svr._sparse = False
    svr.shape_fit_ = tuple(model.shape_fit_)
    svr.fit_status_ = 0
    svr.n_features_in_ = int(model.n_features_in_)
    fit = getattr(model, "fit_result", None)
    svr._num_iter = np.array([0 if fit is None else fit.iterations[0]], dtype=np.int32)
    svr.n_iter_ = int(svr._num_iter[0])
    return svr


def train_random_forest_regression(features, labels, n_estimators):
    """(fitted RandomForestRegressor, mean absolute training error) (reference :229-233), as train_svm_regression."""
    import sklearn.ensemble
    rf = sklearn.ensemble.RandomForestRegressor(n_estimators=n_estimators)
    rf.fit(features, labels)
    X = np.asarray(features, dtype=np.float64)
    pred = regress([rf], "randomforest", X.T, np.zeros(X.shape[1]), np.ones(X.shape[1]))[0]
    return rf, np.mean(np.abs(pred - labels))


def _fit_regressor(features, labels, method_name, param):
    import sklearn.ensemble
    import sklearn.svm
    if method_name == "randomforest":
        model = sklearn.ensemble.RandomForestRegressor(n_estimators=param)
    else:
        model = sklearn.svm.SVR(C=param, kernel="rbf" if method_name == "svm_rbf" else "linear")
    model.fit(features, labels)
    return model


def _check_svr_fit(svm_fit, method_name):
    if svm_fit not in ("sklearn", "device"):
        raise ValueError("svm_fit=%r: 'sklearn' or 'device'" % (svm_fit,))
    if svm_fit == "device" and method_name not in _SVM_TYPES:
        raise ValueError("svm_fit='device' serves the regression methods %s, not %r" % (" and ".join(_SVM_TYPES), method_name))


def _check_forest_regression_fit(forest_fit, method_name):
    if forest_fit not in ("sklearn", "device"):
        raise ValueError("forest_fit=%r: 'sklearn' or 'device'" % (forest_fit,))
    if forest_fit == "device" and method_name != "randomforest":
        raise ValueError("forest_fit='device' serves the regression method 'randomforest', not %r" % (method_name,))


def evaluate_regression(features, labels, n_exp, method_name, params, *, kernel_cache="none", cache_bytes=None, svm_fit="sklearn",
                        forest_fit="sklearn"):
    """Picks the parameter value with the lowest cross-validated squared error (reference :774-855): for every value,
    n_exp random 90 / 10 splits of the standardised samples.  np.random.permutation is consumed and the models are
    fitted in the reference's order (RandomForestRegressor draws from the same global state), by scikit-learn; the
    predictions are deferred: per parameter value the n_exp models x ALL samples go out in one bank launch ("randomforest":
    one traversal per forest), and the test and training errors are picked out on the host with the stored permutations.
    Prints the reference's table; returns (best parameter, its error, its baseline error).  The fits dominate the run
    time: the launch removes the per-vector predict loop and nothing else.
    svm_fit="device" (keyword only; "svm" / "svm_rbf", "randomforest" raises ValueError): ALL len(params) x n_exp permutations
    are drawn up front with np.random.permutation, in the reference's order (an SVR fit draws nothing, so both modes see the
    same splits under one seed), and ONE sweep (svr_split_fit_predict: epsilon-SVR with scikit-learn's defaults epsilon 0.1,
    gamma 'scale', tol 1e-3) fits and scores every split; the training errors come from the solver's gradient.  The errors,
    the baseline, the table and the return value are formed as above.  svm_fit="sklearn" (the default) is the behaviour
    described above, untouched.  kernel_cache / cache_bytes (keyword only, read under svm_fit="device") are
    svr_split_fit_predict's: "gram" solves every split from its resident kernel matrix, with the same bytes out.
    forest_fit="device" (keyword only; "randomforest", any other method raises ValueError): ALL len(params) x n_exp permutations
    are drawn up front, in the reference's order, THEN one forest seed per split with np.random.randint(np.iinfo(np.int32).max), in
    job order (the default mode interleaves every permutation with its forest's own draws, so the two modes see different splits
    under one seed), and ONE sweep (forest_regression_split_fit_predict: RandomForestRegressor(n_estimators=param,
    random_state=seed) per split, on the GPU) fits every forest and scores its test and training rows.  More than 8192 training
    rows raise NotImplementedError.  The errors, the baseline, the table and the return value are formed as above."""
    if method_name not in _REGRESSION_TYPES:
        raise NotImplementedError("regression method %r: 'svm', 'svm_rbf' or 'randomforest'" % (method_name,))
    _check_svr_fit(svm_fit, method_name)
    _check_forest_regression_fit(forest_fit, method_name)
    _cache_mode(kernel_cache, cache_bytes)
    from sklearn.preprocessing import StandardScaler
    features_norm = StandardScaler().fit_transform(features)
    labels = np.asarray(labels)
    n_samples = labels.shape[0]
    n_train = int(round(0.9 * n_samples))
    zeros, ones = np.zeros(features_norm.shape[1]), np.ones(features_norm.shape[1])
    all_samples = np.ascontiguousarray(features_norm.T)
    errors_all, er_train_all, er_base_all = [], [], []
    if svm_fit == "device":                            # one sweep over every split of every parameter value
        all_perms = [[np.random.permutation(range(n_samples)) for _ in range(n_exp)] for _ in params]
        sweep = svr_split_fit_predict(features_norm, labels, [(perm[:n_train], perm[n_train:], zeros, ones, float(param))
                                                              for param, perms in zip(params, all_perms) for perm in perms],
                                      kernel="rbf" if method_name == "svm_rbf" else "linear", train_pred=True,
                                      kernel_cache=kernel_cache, cache_bytes=cache_bytes)
    if forest_fit == "device":                         # likewise: every permutation, then every forest's seed, then one sweep
        _check_targets(labels)
        _check_tree_rows(n_train, "a training split")
        all_perms = [[np.random.permutation(range(n_samples)) for _ in range(n_exp)] for _ in params]
        seeds = [[int(np.random.randint(np.iinfo(np.int32).max)) for _ in range(n_exp)] for _ in params]
        sweep = forest_regression_split_fit_predict(
            features_norm, labels, [(perm[:n_train], perm[n_train:], zeros, ones, (int(param), seed))
                                    for param, perms, srow in zip(params, all_perms, seeds) for perm, seed in zip(perms, srow)], train_pred=True)
    for p, param in enumerate(params):
        if svm_fit == "device" or forest_fit == "device":
            perms = all_perms[p]
            picked = [sweep.job(p * n_exp + e)[:2] for e in range(n_exp)]          # (test, training) predictions per experiment
        else:
            perms, models = [], []
            for _ in range(n_exp):
                perm = np.random.permutation(range(n_samples))
                models.append(_fit_regressor(features_norm[perm[:n_train]], [labels[i] for i in perm[:n_train]], method_name, param))
                perms.append(perm)
            pred = regress(models, method_name, all_samples, zeros, ones)           # [n_exp][n_samples]
            picked = [(pred[e, perm[n_train:]], pred[e, perm[:n_train]]) for e, perm in enumerate(perms)]
        errors, errors_train, errors_base = [], [], []
        for (pred_test, pred_train), perm in zip(picked, perms):
            train, test = perm[:n_train], perm[n_train:]
            baseline = np.mean([labels[i] for i in train])
            errors.append(np.array([(pred_test[k] - labels[i]) * (pred_test[k] - labels[i]) for k, i in enumerate(test)]).mean())
            errors_base.append(np.array([(baseline - labels[i]) * (baseline - labels[i]) for i in test]).mean())
            errors_train.append(np.mean(np.abs(pred_train - labels[train])))
        errors_all.append(np.array(errors).mean())
        er_train_all.append(np.array(errors_train).mean())
        er_base_all.append(np.array(errors_base).mean())
    best = int(np.argmin(errors_all))
    print("{0:s}\t\t{1:s}\t\t{2:s}\t\t{3:s}".format("Param", "MSE", "T-MSE", "R-MSE"))
    for i in range(len(errors_all)):
        print("{0:.4f}\t\t{1:.2f}\t\t{2:.2f}\t\t{3:.2f}".format(params[i], errors_all[i], er_train_all[i], er_base_all[i]), end="")
        print("\t\t best" if i == best else "")
    return params[best], errors_all[best], er_base_all[best]


def save_parameters(path, *parameters):
    """The MEANS file of a model: the parameters pickled one after the other (reference :364-367)."""
    with open(path, "wb") as fo:
        for p in parameters:
            cPickle.dump(p, fo, protocol=cPickle.HIGHEST_PROTOCOL)


def feature_extraction_train_regression(folder_name, mid_window, mid_step, short_window, short_step, model_type, model_name,
                                        compute_beat=False, *, svm_fit="sklearn", forest_fit="sklearn", final_fit="sklearn",
                                        kernel_cache="none"):
    """Trains one regression model per CSV file of a folder of audio files (reference :370-489): every `<task>.csv` pairs
    file names with target values; features come from multiple_directory_feature_extraction (GPU), the parameter from
    evaluate_regression, the final fit from scikit-learn; `model_name_<task>` and `model_name_<task>MEANS` are written as
    the reference writes them.  svm_fit (keyword only) goes to evaluate_regression: "device" tunes C on the GPU; the final fit
    and the model file, a pickled SVR, stay scikit-learn's.  forest_fit (keyword only, "randomforest") goes to evaluate_regression
    too; with "device" the final fit is train_random_forest_regression_device and the model file is the pickled
    to_sklearn_forest_regressor of its arrays, a real RandomForestRegressor that load_model(..., is_regression=True) and
    file_regression read unchanged.  final_fit="device" (keyword only; "svm" / "svm_rbf", any other type raises ValueError):
    the final model is to_sklearn_svr(train_svm_regression_device(...)) at the chosen C, a real SVR pickled in the reference's
    format; svm_fit="device" alone keeps writing scikit-learn's fit.  kernel_cache (keyword only) goes to evaluate_regression
    and to that final fit.  Returns (errors, baseline errors, best parameters)."""
    _check_svr_fit(svm_fit, model_type)
    _check_forest_regression_fit(forest_fit, model_type)
    if final_fit not in ("sklearn", "device"):
        raise ValueError("final_fit=%r: 'sklearn' or 'device'" % (final_fit,))
    if final_fit == "device" and model_type not in _SVM_TYPES:
        raise ValueError("final_fit='device' serves the regression methods %s, not %r" % (" and ".join(_SVM_TYPES), model_type))
    _cache_mode(kernel_cache, None)
    import csv
    import glob
    import ntpath
    from sklearn.preprocessing import StandardScaler
    features, _, filenames = aF.multiple_directory_feature_extraction([folder_name], mid_window, mid_step, short_window,
                                                                      short_step, compute_beat=compute_beat)
    features = features[0]
    filenames = [ntpath.basename(f) for f in filenames[0]]
    task_features, task_labels, task_names = [], [], []
    for path in glob.glob(folder_name + os.sep + "*.csv"):
        rows, values = [], []
        with open(path, "rt") as fo:
            for row in csv.reader(fo, delimiter=",", quotechar="|"):
                if len(row) != 2:
                    print("Warning: Row with unknown format in regression file")
                elif row[0] in filenames:
                    values.append(float(row[1]))
                    rows.append(features[filenames.index(row[0]), :])
                else:
                    print("Warning: {} not found in list of files.".format(row[0]))
        task_features.append(np.array(rows))
        task_labels.append(np.array(values))
        task_names.append(ntpath.basename(path).replace(".csv", ""))
        if len(features) == 0:
            print("ERROR: No data found in any input folder!")
            return
    if model_type in _SVM_TYPES:
        model_params = np.array([0.001, 0.005, 0.01, 0.05, 0.1, 0.25, 0.5, 1.0, 5.0, 10.0])
    elif model_type == "randomforest":
        model_params = np.array([5, 10, 25, 50, 100])
    errors, errors_base, best_params = [], [], []
    for X, y, name in zip(task_features, task_labels, task_names):
        print("Regression task " + name)
        best, error, base_error = evaluate_regression(X, y, 100, model_type, model_params, svm_fit=svm_fit, forest_fit=forest_fit,
                                                      kernel_cache=kernel_cache)
        errors.append(error)
        errors_base.append(base_error)
        best_params.append(best)
        print("Selected params: {0:.5f}".format(best))
        scaler = StandardScaler()
        X_norm = scaler.fit_transform(X)
        if model_type in _REGRESSION_TYPES:
            if forest_fit == "device":
                model = to_sklearn_forest_regressor(train_random_forest_regression_device(X_norm, y, int(best))[0])
            elif final_fit == "device":
                model = to_sklearn_svr(train_svm_regression_device(X_norm, y, best, "rbf" if model_type == "svm_rbf" else "linear",
                                                                   kernel_cache=kernel_cache)[0])
            else:
                model = _fit_regressor(X_norm, y, model_type, best)
            with open(model_name + "_" + name, "wb") as fo:
                cPickle.dump(model, fo)
            save_parameters(model_name + "_" + name + "MEANS", scaler.mean_.tolist(), scaler.scale_.tolist(), mid_window,
                            mid_step, short_window, short_step, compute_beat)
    return errors, errors_base, best_params


def file_regression_signals(signals, sampling_rate, models, means, stds, mid_window, mid_step, short_window, short_step,
                            compute_beat, model_type="svm_rbf"):
    """file_regression for many mono signals of one sampling rate and loaded models: the clips go through ONE batched
    mid-term (+ beat) plan, the long-term vectors through ONE regression launch (regress).  There is no short-file clamp
    of mid_window here (reference :1127-1131, unlike file_classification).  Returns [n_signals][n_models]."""
    models = list(models)
    if len(signals) == 0:
        return np.zeros((0, len(models)))
    feats = _long_term_vectors(signals, sampling_rate, mid_window, mid_step, short_window, short_step, compute_beat, False)
    return np.ascontiguousarray(regress(models, model_type, feats, means, stds).T)


def file_regression_signal(signal, sampling_rate, models, means, stds, mid_window, mid_step, short_window, short_step,
                           compute_beat, model_type="svm_rbf"):
    """file_regression on a mono signal and loaded models: the regression results [n_models] (a batch of one clip)."""
    return file_regression_signals([signal], sampling_rate, models, means, stds, mid_window, mid_step, short_window,
                                   short_step, compute_beat, model_type)[0]


def _regression_models(model_name):
    """file_regression's model files (reference :1106-1114): every model_name_* that is no MEANS file, and the task names
    (the text after the last underscore)."""
    import glob
    paths = [r for r in glob.glob(model_name + "_*") if r[-5::] != "MEANS"]
    return paths, [r[r.rfind("_") + 1::] for r in paths]


def _load_regression_models(paths):
    """(models, means, stds, window parameters of the FIRST model) or None when a model file is missing."""
    models, means, stds = [], [], []
    params = load_model(paths[0], True)[3:]
    for r in paths:
        if not os.path.isfile(r):
            print("fileClassification: input model_name not found!")
            return None
        model, mean, std = load_model(r, True)[:3]
        models.append(model)
        means.append(mean)
        stds.append(std)
    return models, np.array(means), np.array(stds), params


def file_regression(input_file, model_name, model_type):
    """(regression results, task names) of one audio file for every model model_name_<task> (reference :1099-1151); the
    reference's error return (-1, -1, -1) for a missing file or model."""
    if not os.path.isfile(input_file):
        print("fileClassification: wav file not found!")
        return -1, -1, -1
    paths, names = _regression_models(model_name)
    if model_type not in _REGRESSION_TYPES:
        raise NotImplementedError("regression model type %r: the GPU path serves 'svm', 'svm_rbf' and 'randomforest'" % (model_type,))
    loaded = _load_regression_models(paths)
    if loaded is None:
        return -1, -1, -1
    models, means, stds, (mid_window, mid_step, short_window, short_step, compute_beat) = loaded
    sampling_rate, signal = audioBasicIO.read_audio_file(input_file)
    signal = audioBasicIO.stereo_to_mono(signal)
    R = file_regression_signal(signal, sampling_rate, models, means, stds, mid_window, mid_step, short_window, short_step,
                               compute_beat, model_type)
    return list(R), names


def file_regression_batch(files, model_name, model_type):
    """file_regression over many files with one set of models: a list of (results, task names) per file, equal to one-file
    calls.  Files are grouped by sampling rate; each group is one batched mid-term plan and one regression launch.
    Missing / unreadable files give the reference's (-1, -1, -1)."""
    out = [(-1, -1, -1)] * len(files)
    present = [i for i, f in enumerate(files) if os.path.isfile(f)]
    for i in range(len(files)):
        if i not in present:
            print("fileClassification: wav file not found!")
    if not present:
        return out
    if model_type not in _REGRESSION_TYPES:
        raise NotImplementedError("regression model type %r: the GPU path serves 'svm', 'svm_rbf' and 'randomforest'" % (model_type,))
    paths, names = _regression_models(model_name)
    loaded = _load_regression_models(paths)
    if loaded is None:
        return out
    models, means, stds, (mid_window, mid_step, short_window, short_step, compute_beat) = loaded
    for fs, members in _read_by_sampling_rate(files, present).items():
        R = file_regression_signals([s for _, s in members], fs, models, means, stds, mid_window, mid_step, short_window,
                                    short_step, compute_beat, model_type)
        for j, (i, _) in enumerate(members):
            out[i] = (list(R[j]), names)
    return out
