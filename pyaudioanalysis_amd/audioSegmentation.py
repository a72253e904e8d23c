"""GPU drop-ins for the numerically heavy functions of pyAudioAnalysis.audioSegmentation.

    self_similarity_matrix(feature_vectors)                      audioSegmentation.py:40-55
    music_thumbnailing(signal, sampling_rate, short_window=1.0,  audioSegmentation.py:1096-1190
                       short_step=0.5, thumb_size=10.0, limit_1=0, limit_2=1)
    silence_removal(signal, sampling_rate, st_win, st_step,      audioSegmentation.py:672-815
                    smooth_window=0.5, weight=0.5, plot=False)

Same names, argument meaning and return values as the reference.  Everything numeric runs in libpaa_hip.so
(standardisation, FP64 matrix-core Gram matrix, diagonal filter, masks, arg-max; short-term features and the per-frame
SVM probability of silence_removal); there is no CPU fallback for those.  `music_thumbnailing` keeps the short-term
features and the similarity matrix in HBM: only the filtered matrix it returns comes back to the host.
music_thumbnailing_batch / music_thumbnailing_files do that for a collection of clips in one call: one batched plan, the stages of
all clips one launch each, the arg-max cell grown on the device, 48 bytes per clip back (self_similarity_batch,
thumbnail_filter_batch and thumbnail_batch give the stages alone); clip i equals its own music_thumbnailing call bit for bit.
`silence_removal` trains its two-class SVM exactly where the reference does -- with scikit-learn (:739,
audioTrainTest.train_svm) -- and replaces the per-frame predict_proba loop (:744-748) by one kernel over all frames
(svm_onset_probability); with svm_fit="device" the SVM is trained on the GPU instead (audioTrainTest.train_svm_device: the full
fit, libsvm's five cross-validation fits and the sigmoid fit) and scikit-learn is not needed.  silence_removal_batch /
silence_removal_files do that for many clips in one call, on the GPU end to end: energy selection, training sets and scalers, the
fits of all clips as one solver batch, probabilities, smoothing and thresholds (onset_training_sets and onset_activity give the
stages around the fit alone).  The HMM segmenter (train_hmm_compute_statistics, train_hmm_from_file / _from_directory, save_hmm,
hmm_segmentation, :287-492) runs on the GPU as well: class GaussianHmm stands in for hmmlearn's GaussianHMM (hmmlearn is not
needed, also not to read a model file the reference wrote).  Speaker diarization (speaker_diarization, diarize_features,
evaluate_speaker_diarization, speaker_diarization_evaluation, :251-284, :815-1090) runs its standardisation, k-means sweep and
silhouettes on the GPU as well.  Its LDA branch (lda_dim > 0, :880-934) has entry points of its own -- speaker_diarization_lda,
speaker_diarization_lda_signal, lda_fit_device / lda_transform_device / lda_fit_transform: class statistics, within-class
Gram matrix and projection on the GPU, two eigenproblems of at most 256 x 256 with numpy.linalg.eigh on the host;
speaker_diarization(lda_dim > 0) itself refuses and names them.
"""
import contextlib
import ctypes as C
import time

import numpy as np

from . import _ffi
from . import audioBasicIO


def self_similarity_matrix(feature_vectors):
    """(nDims x nVectors) feature matrix -> (nVectors x nVectors) cosine self-similarity of the standardised
    columns (audioSegmentation.py:40-55)."""
    F = np.ascontiguousarray(np.asarray(feature_vectors, dtype=np.float64))
    if F.ndim != 2 or F.shape[0] < 1 or F.shape[1] < 1:
        raise ValueError("feature_vectors must be a non-empty (nDims x nVectors) matrix")
    sim = _ffi.result_array((F.shape[1], F.shape[1]))
    _ffi.check(_ffi.lib().paa_self_similarity_f64(_ffi.as_f64p(F), F.shape[0], F.shape[1], _ffi.as_f64p(sim)))
    return sim


def _grow_thumbnail(filtered, rows, cols, m_filter):
    # extend the arg-max cell along its diagonal until it spans m_filter cells (:1167-1182)
    i1 = i2 = int(rows)
    j1 = j2 = int(cols)
    last_r, last_c = filtered.shape[0] - 2, filtered.shape[1] - 2
    while i2 - i1 < m_filter:
        if i1 <= 0 or j1 <= 0 or i2 >= last_r or j2 >= last_c:
            break
        if filtered[i1 - 1, j1 - 1] > filtered[i2 + 1, j2 + 1]:
            i1, j1 = i1 - 1, j1 - 1
        else:
            i2, j2 = i2 + 1, j2 + 1
    return i1, i2, j1, j2


def music_thumbnailing(signal, sampling_rate, short_window=1.0, short_step=0.5, thumb_size=10.0,
                       limit_1=0, limit_2=1):
    """Returns (A1, A2, B1, B2, filtered similarity matrix): start / end of the two thumbnail instances in seconds
    (audioSegmentation.py:1096-1190)."""
    lib = _ffi.lib()
    signal = audioBasicIO.stereo_to_mono(signal)
    kind, sig = _ffi.classify_signal(signal)
    window, step = int(sampling_rate * short_window), int(sampling_rate * short_step)     # int() of :563-564
    n_frames = int(lib.paa_num_frames(len(sig), window, step)) if window > 0 and step > 0 else 0
    if n_frames < 1:
        raise ValueError("need at least one array to concatenate")          # ShortTermFeatures.py:684
    m_filter = int(round(thumb_size / short_step))                           # :1142
    R = int(lib.paa_thumbnail_rows(n_frames, m_filter))
    if R < 1:
        raise ValueError("%d feature vectors are fewer than the thumbnail filter length %d (the reference's "
                         "convolve2d silently swaps its operands in that case)" % (n_frames, m_filter))
    offsets = np.array([0, len(sig)], dtype=np.int64)
    plan = _ffi.Plan(offsets, sampling_rate, window, step, deltas=True, sample_kind=kind)
    d_in = d_st = d_sim = d_filt = None
    try:
        d_in = _ffi.DeviceBuffer.from_host(sig)
        d_st = _ffi.DeviceBuffer(plan.out_doubles * 8)
        plan.execute(d_in, d_st)
        d_sim = _ffi.DeviceBuffer(n_frames * n_frames * 8)
        _ffi.check(lib.paa_dev_self_similarity(d_st.ptr, plan.F, n_frames, n_frames, d_sim.ptr))
        d_filt = _ffi.DeviceBuffer(R * R * 8)
        pos = np.zeros(2, dtype=np.int64)
        _ffi.check(lib.paa_dev_thumbnail_filter(d_sim.ptr, n_frames, m_filter, 5.0 / short_step, float(limit_1),
                                                float(limit_2), d_filt.ptr, _ffi.as_i64p(pos)))
        filtered = d_filt.to_host(np.float64, R * R).reshape(R, R)
    finally:
        for b in (d_in, d_st, d_sim, d_filt):
            if b is not None:
                b.free()
        plan.destroy()
    i1, i2, j1, j2 = _grow_thumbnail(filtered, pos[0], pos[1], m_filter)
    return short_step * i1, short_step * i2, short_step * j1, short_step * j2, filtered


# ---------------------------------------------------------------------------------------------------------
# music thumbnailing for a batch of clips (the stages of :40-55 and :1141-1182 as one launch each over all clips)
# ---------------------------------------------------------------------------------------------------------
def _feature_mats(mats):
    """list of (n_dims x T_c) matrices of one n_dims -> (contiguous float64 matrices, n_vec int64 [n], n_dims)"""
    mats = [np.ascontiguousarray(np.asarray(f, dtype=np.float64)) for f in mats]
    for c, f in enumerate(mats):
        if f.ndim != 2 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("clip %d: feature_vectors must be a non-empty (nDims x nVectors) matrix" % c)
        if f.shape[0] != mats[0].shape[0]:
            raise ValueError("clip %d: %d feature rows, clip 0 has %d" % (c, f.shape[0], mats[0].shape[0]))
    return mats, np.array([f.shape[1] for f in mats], dtype=np.int64), (mats[0].shape[0] if mats else 0)


def _pack(arrays):
    return np.concatenate([a.reshape(-1) for a in arrays]) if len(arrays) > 1 else arrays[0].reshape(-1)


def _check_filter_length(n_vec, m_filter):
    m_filter = int(m_filter)
    if m_filter < 1:
        raise ValueError("thumbnail filter length %d" % m_filter)
    for c, t in enumerate(n_vec):
        if t < m_filter:
            raise ValueError("clip %d: %d feature vectors are fewer than the thumbnail filter length %d" % (c, t, m_filter))
    return m_filter


def _split_squares(flat, sizes):
    out, at = [], 0
    for r in sizes:
        out.append(flat[at:at + r * r].reshape(r, r))
        at += r * r
    return out


def _thumb_outputs(n_vec, m_filter, want_filtered):
    """(pos [n][2], bounds [n][4], filt or None, R [n]) of one thumbnail batch call"""
    R = [int(t) - m_filter + 1 for t in n_vec]
    filt = _ffi.result_array((sum(r * r for r in R),)) if want_filtered else None
    return np.zeros((len(R), 2), dtype=np.int64), np.zeros((len(R), 4), dtype=np.int64), filt, R


def _thumb_records(pos, bounds, filt, R):
    """per clip ((row, column), (i1, i2, j1, j2), filtered or None)"""
    mats = _split_squares(filt, R) if filt is not None else [None] * len(R)
    return [(tuple(int(v) for v in pos[c]), tuple(int(v) for v in bounds[c]), mats[c]) for c in range(len(R))]


def self_similarity_batch(mats, *, chunk_bytes=None):
    """self_similarity_matrix for a list of (nDims x T_c) matrices of one nDims in one library call: the Gram tiles of all
    clips are one launch.  Returns the T_c x T_c matrices; clip i equals self_similarity_matrix(mats[i]) bit for bit."""
    mats, n_vec, n_dims = _feature_mats(mats)
    if not mats:
        return []
    sim = _ffi.result_array((int((n_vec * n_vec).sum()),))
    _ffi.check(_ffi.lib().paa_self_similarity_batch_f64(_ffi.as_f64p(_pack(mats)), n_dims, len(mats), _ffi.as_i64p(n_vec),
                                                        int(chunk_bytes or 0), _ffi.as_f64p(sim)))
    return _split_squares(sim, [int(t) for t in n_vec])


def thumbnail_filter_batch(sims, m_filter, band, limit_1=0, limit_2=1, *, return_filtered=True, chunk_bytes=None):
    """The matrix part of music_thumbnailing after the similarity matrix, for a list of symmetric T_c x T_c matrices: diagonal
    filter of m_filter cells, masks (band is the reference's 5.0 / short_step), arg-max and the grown thumbnail.  Returns per
    clip (filtered, (row, column), (i1, i2, j1, j2)), without `filtered` when return_filtered is False."""
    sims = [np.ascontiguousarray(np.asarray(s, dtype=np.float64)) for s in sims]
    for c, s in enumerate(sims):
        if s.ndim != 2 or s.shape[0] != s.shape[1] or s.shape[0] < 1:
            raise ValueError("clip %d: a similarity matrix is square and not empty (shape %s)" % (c, s.shape))
    if not sims:
        return []
    n_vec = np.array([s.shape[0] for s in sims], dtype=np.int64)
    m_filter = _check_filter_length(n_vec, m_filter)
    pos, bounds, filt, R = _thumb_outputs(n_vec, m_filter, return_filtered)
    _ffi.check(_ffi.lib().paa_thumbnail_filter_batch_f64(_ffi.as_f64p(_pack(sims)), len(sims), _ffi.as_i64p(n_vec), m_filter, float(band),
                                                         float(limit_1), float(limit_2), int(chunk_bytes or 0), _ffi.as_i64p(pos),
                                                         _ffi.as_i64p(bounds), _ffi.as_f64p(filt) if filt is not None else None))
    return [(f, p, b) if return_filtered else (p, b) for p, b, f in _thumb_records(pos, bounds, filt, R)]


def thumbnail_batch(mats, m_filter, band, limit_1=0, limit_2=1, *, return_filtered=True, chunk_bytes=None):
    """self_similarity_batch and thumbnail_filter_batch in one call, the similarity matrices staying in device memory: per clip
    (filtered, (row, column), (i1, i2, j1, j2)) from its (nDims x T_c) feature matrix."""
    mats, n_vec, n_dims = _feature_mats(mats)
    if not mats:
        return []
    m_filter = _check_filter_length(n_vec, m_filter)
    pos, bounds, filt, R = _thumb_outputs(n_vec, m_filter, return_filtered)
    _ffi.check(_ffi.lib().paa_thumbnail_batch_f64(_ffi.as_f64p(_pack(mats)), n_dims, len(mats), _ffi.as_i64p(n_vec), m_filter, float(band),
                                                  float(limit_1), float(limit_2), int(chunk_bytes or 0), _ffi.as_i64p(pos),
                                                  _ffi.as_i64p(bounds), _ffi.as_f64p(filt) if filt is not None else None))
    return [(f, p, b) if return_filtered else (p, b) for p, b, f in _thumb_records(pos, bounds, filt, R)]


def _thumb_plan(lengths, sampling_rate, short_window, short_step, thumb_size):
    """The argument half of music_thumbnailing_batch, without the device: (window, step, m_filter, frames) or the ValueError
    of the first clip that cannot be served."""
    window, step = int(sampling_rate * short_window), int(sampling_rate * short_step)     # int() of :563-564
    if window < 2 or step < 1:
        raise ValueError("short_window = %r, short_step = %r at %r Hz: a window of %d and a step of %d samples"
                         % (short_window, short_step, sampling_rate, window, step))
    m_filter = int(round(thumb_size / short_step))                           # :1142
    if m_filter < 1:
        raise ValueError("thumb_size = %r, short_step = %r: a thumbnail filter of %d cells" % (thumb_size, short_step, m_filter))
    frames = [(int(m) - window) // step + 1 if int(m) >= window else 0 for m in lengths]
    for c, t in enumerate(frames):
        if t < 1:
            raise ValueError("clip %d: need at least one array to concatenate (%d samples, a window of %d)"
                             % (c, lengths[c], window))                       # ShortTermFeatures.py:684
        if t < m_filter:
            raise ValueError("clip %d: %d feature vectors are fewer than the thumbnail filter length %d (the reference's "
                             "convolve2d silently swaps its operands in that case)" % (c, t, m_filter))
    return window, step, m_filter, np.array(frames, dtype=np.int64)


def _thumb_group(clips, as_i16, sampling_rate, window, step, frames, m_filter, band, limit_1, limit_2, want_filtered, chunk_bytes):
    """The call of paa_music_thumbnail_batch_* for clips of one sample type: per clip ((row, column), (i1, i2, j1, j2), filtered)"""
    n = len(clips)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([c.shape[0] for c in clips], out=offsets[1:])
    ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in clips])               # one pointer per clip: no packing copy on the host
    pos, bounds, filt, R = _thumb_outputs(frames, m_filter, want_filtered)
    lib = _ffi.lib()
    fn = lib.paa_music_thumbnail_batch_ptrs_i16 if as_i16 else lib.paa_music_thumbnail_batch_ptrs_f64
    _ffi.check(fn(ptrs, _ffi.as_i64p(offsets), n, float(sampling_rate), window, step,
                  m_filter, float(band), float(limit_1), float(limit_2), int(chunk_bytes or 0), _ffi.as_i64p(pos), _ffi.as_i64p(bounds),
                  _ffi.as_f64p(filt) if filt is not None else None))
    return _thumb_records(pos, bounds, filt, R)


def _thumb_batch(monos, sampling_rate, short_window, short_step, thumb_size, limit_1, limit_2, want_filtered, chunk_bytes):
    """music_thumbnailing_batch on mono clips whose arguments have passed: the int16 clips and the others are one library call
    each, so that every clip takes the sample path of its own single call.  Records in clip order."""
    window, step, m_filter, frames = _thumb_plan([m.shape[0] for m in monos], sampling_rate, short_window, short_step, thumb_size)
    out = [None] * len(monos)
    for as_i16 in (True, False):
        ids = [c for c, m in enumerate(monos) if (m.dtype == np.int16) == as_i16]
        if not ids:
            continue
        clips = [np.ascontiguousarray(monos[c] if as_i16 else np.double(monos[c])) for c in ids]
        try:
            records = _thumb_group(clips, as_i16, sampling_rate, window, step, frames[ids], m_filter, 5.0 / short_step, limit_1, limit_2,
                                   want_filtered, chunk_bytes)
        except (ValueError, NotImplementedError) as exc:
            raise _as_path_index(exc, ids)
        for c, r in zip(ids, records):
            out[c] = r
    return out


def _thumb_result(record, short_step, return_filtered, return_details):
    pos, (i1, i2, j1, j2), filtered = record
    res = (short_step * i1, short_step * i2, short_step * j1, short_step * j2)
    if return_filtered:
        res += (filtered,)
    if return_details:
        res += (pos,)
    return res


def _mono_clips(signals):
    monos = [np.asarray(audioBasicIO.stereo_to_mono(s)) for s in signals]
    for c, m in enumerate(monos):
        if m.ndim != 1:
            raise ValueError("clip %d: a signal of %d dimensions (mono, or two channels)" % (c, m.ndim))
    return monos


def music_thumbnailing_batch(signals, sampling_rate, short_window=1.0, short_step=0.5, thumb_size=10.0, limit_1=0, limit_2=1, *,
                             return_filtered=False, return_details=False, chunk_bytes=None):
    """music_thumbnailing for a list of clips of ONE sampling rate, on the GPU end to end: the short-term matrices of one batched
    plan stay in device memory; standardisation, the Gram tiles of all clips on the FP64 matrix cores, the diagonal filter,
    the folds and the growth of the arg-max cell are one launch each over the whole batch, and 48 bytes per clip come back.
    Returns one (A1, A2, B1, B2) per clip in seconds, exactly what music_thumbnailing returns for that clip alone;
    return_filtered=True appends the filtered matrix (then it is copied back as well), return_details=True the (row, column)
    of the arg-max.  Each clip goes through audioBasicIO.stereo_to_mono; int16 clips travel as int16, the others through
    np.double (two library calls when both kinds are present).  chunk_bytes: a bound below the library's 1 GiB for the device
    scratch of one chunk of clips (tests); no result depends on it.  An empty list returns [].

    ValueError names the clip and comes before any device work: a clip shorter than one window (the reference's "need at
    least one array to concatenate"), or with fewer vectors than round(thumb_size / short_step).  NotImplementedError for a
    clip past self_similarity_matrix's size bound."""
    signals = list(signals)
    if not signals:
        return []
    records = _thumb_batch(_mono_clips(signals), sampling_rate, short_window, short_step, thumb_size, limit_1, limit_2, return_filtered,
                           chunk_bytes)
    return [_thumb_result(r, short_step, return_filtered, return_details) for r in records]


def music_thumbnailing_files(paths, short_window=1.0, short_step=0.5, thumb_size=10.0, limit_1=0, limit_2=1, *,
                             return_filtered=False, return_details=False):
    """music_thumbnailing_batch over audio files: they are read and grouped by sampling rate, one device batch per rate, and
    the results come back in path order.  A file that cannot be read raises ValueError naming its index; the arguments of
    EVERY file are checked before the device is touched."""
    paths = list(paths)
    groups = {}
    for i, path in enumerate(paths):
        fs, sig = audioBasicIO.read_audio_file(path)
        if fs <= 0:
            raise ValueError("file %d (%s) cannot be read" % (i, path))
        groups.setdefault(fs, []).append((i, sig))
    monos = {}
    for fs, members in groups.items():
        ids = [i for i, _ in members]
        try:
            monos[fs] = _mono_clips([s for _, s in members])
            _thumb_plan([m.shape[0] for m in monos[fs]], fs, short_window, short_step, thumb_size)
        except ValueError as exc:
            raise _as_path_index(exc, ids)
    out = [None] * len(paths)
    for fs, members in groups.items():
        ids = [i for i, _ in members]
        try:
            records = _thumb_batch(monos[fs], fs, short_window, short_step, thumb_size, limit_1, limit_2, return_filtered, None)
        except (ValueError, NotImplementedError) as exc:
            raise _as_path_index(exc, ids)
        for i, r in zip(ids, records):
            out[i] = _thumb_result(r, short_step, return_filtered, return_details)
    return out


# ---------------------------------------------------------------------------------------------------------
# silence removal (reference :672-815)
# ---------------------------------------------------------------------------------------------------------
def smooth_moving_avg(signal, window=11):
    """Box-filter smoothing of a 1-D sequence whose ends are continued by point reflection about the first / last
    sample (what the reference's helper computes, audioSegmentation.py:25-37): out[i] is the mean of `width`
    consecutive entries of the extended sequence, the block ending (width - 1) // 2 entries after position i.
    width = int(window); sequences are returned untouched for width < 3 (:31-32); ValueError for anything that is
    not one-dimensional or is shorter than the width (:27-30)."""
    width = int(window)
    seq = signal
    if seq.ndim != 1:
        raise ValueError("smooth_moving_avg needs a one-dimensional sequence, got %d dimensions" % seq.ndim)
    n = seq.size
    if n < width:
        raise ValueError("Input vector needs to be bigger than window size.")
    if width < 3:
        return signal
    # point reflections: `width` entries in front (seq[width-1] .. seq[0] mirrored about seq[0]), width - 1 behind
    lead = 2.0 * seq[0] - seq[:width][::-1]
    trail = 2.0 * seq[-1] - seq[n - width + 1:][::-1]
    extended = np.concatenate((lead, seq, trail))
    box = np.full(width, 1.0) / float(width)
    # 'valid' block means m[k] = mean(extended[k : k + width]); out[i] uses the block that ends at extended index
    # width + i + (width - 1) // 2, i.e. k = i + 1 + (width - 1) // 2  (np.convolve(.., 'same') of the reference, cropped)
    first = 1 + (width - 1) // 2
    return np.convolve(extended, box, mode="valid")[first:first + n]


def svm_onset_probability(st_feats, mean, std, svm):
    """svm.predict_proba((st_feats[:, i] - mean) / std)[0][1] for every frame i (reference :744-748) in one kernel.

    svm: a TRAINED binary scikit-learn SVC with probability=True (kernel 'linear' or 'rbf'); only its arrays are read
    (support_vectors_, dual_coef_, intercept_, probA_, probB_, kernel, _gamma)."""
    F = np.ascontiguousarray(np.asarray(st_feats, dtype=np.float64))
    if F.ndim != 2:
        raise ValueError("st_feats must be (n_feats x n_frames)")
    kernel = getattr(svm, "kernel", "linear")
    if kernel not in ("linear", "rbf"):
        raise NotImplementedError("SVC kernel %r (the reference trains linear SVMs here, audioTrainTest.py:152)" % (kernel,))
    if len(getattr(svm, "classes_", (0, 1))) != 2:
        raise ValueError("a two-class SVC is required")
    sv = np.ascontiguousarray(svm.support_vectors_, dtype=np.float64)
    coef = np.ascontiguousarray(np.asarray(svm.dual_coef_, dtype=np.float64).reshape(-1))
    if kernel == "linear":
        # <sum_i coef_i sv_i, x>: fold the support vectors into one weight vector (same value up to rounding order)
        sv = np.ascontiguousarray((coef[:, None] * sv).sum(axis=0, keepdims=True))
        coef = np.ones(1)
    mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(-1))
    std = np.ascontiguousarray(np.asarray(std, dtype=np.float64).reshape(-1))
    if sv.shape[1] != F.shape[0] or mean.shape[0] != F.shape[0] or std.shape[0] != F.shape[0]:
        raise ValueError("feature dimension mismatch between st_feats, the scaler and the SVM")
    prob = np.empty(F.shape[1])
    gamma = float(svm._gamma) if kernel == "rbf" else 0.0
    _ffi.check(_ffi.lib().paa_svm_binary_proba_f64(
        _ffi.as_f64p(F), F.shape[0], F.shape[1], _ffi.as_f64p(mean), _ffi.as_f64p(std), _ffi.as_f64p(sv),
        _ffi.as_f64p(coef), sv.shape[0], float(np.asarray(svm.intercept_).reshape(-1)[0]), gamma,
        float(np.asarray(svm.probA_).reshape(-1)[0]), float(np.asarray(svm.probB_).reshape(-1)[0]), _ffi.as_f64p(prob)))
    return prob


def _train_onset_svm(low_energy, high_energy):
    """Steps of reference :727-739: features_to_matrix, StandardScaler, train_svm(.., 1.0) -- scikit-learn's job."""
    try:
        import sklearn.svm
        from sklearn.preprocessing import StandardScaler
    except ImportError as exc:       # the reference needs it at the same place
        raise ImportError("silence_removal trains its SVM with scikit-learn (audioSegmentation.py:733-739): %s" % exc)
    features = np.vstack([low_energy, high_energy])
    labels = np.append(np.zeros(low_energy.shape[0]), np.ones(high_energy.shape[0]))     # audioTrainTest.features_to_matrix
    scaler = StandardScaler()
    features_norm = scaler.fit_transform(features)
    svm = sklearn.svm.SVC(C=1.0, kernel='linear', probability=True, gamma='auto')         # audioTrainTest.py:152-154
    svm.fit(features_norm, labels)
    return svm, scaler.mean_, scaler.scale_


def _energy_extremes(st_feats):
    """Columns (frames) of the short-term matrix that fall into the quietest / loudest tenth by energy (row 1):
    thresholds are the means of the lowest and of the highest tenth of the sorted energies -- the loudest frame itself
    left out of the upper mean, as in the reference -- plus 1e-15 (audioSegmentation.py:713-728)."""
    energy = st_feats[1]
    ranked = np.sort(energy)
    tenth = int(ranked.size / 10)
    quiet_limit = ranked[:tenth].mean() + 1e-15
    loud_limit = ranked[-tenth:-1].mean() + 1e-15
    return st_feats[:, energy <= quiet_limit], st_feats[:, energy >= loud_limit]


def _onset_threshold(prob, weight):
    """Weighted mix of the mean of the lowest tenth and the mean of the highest tenth of the smoothed probabilities
    (audioSegmentation.py:753-759; the low part is scaled before it is averaged, the high part after)."""
    ranked = np.sort(prob)
    tenth = int(ranked.size / 10)
    return ((1 - weight) * ranked[:tenth]).mean() + weight * ranked[-tenth:].mean()


def _onset_segments(active, st_step, min_duration=0.2):
    """Frame indices above the threshold -> [start, end] limits in seconds (audioSegmentation.py:764-791).

    Indices whose neighbours are at most 2 frames apart belong to one segment; the list is cut where np.diff exceeds 2.
    A segment is kept when it lasts longer than min_duration seconds (:786-790) -- which also removes every one-frame
    segment, so the reference's habit of never opening a segment at the very last index (:770-771) changes nothing."""
    active = np.asarray(active)
    if active.size == 0:
        return []
    cuts = np.flatnonzero(np.diff(active) > 2) + 1
    firsts = active[np.concatenate(([0], cuts))]
    lasts = active[np.concatenate((cuts - 1, [active.size - 1]))]
    limits = [[lo * st_step, hi * st_step] for lo, hi in zip(firsts, lasts)]
    return [seg for seg in limits if seg[1] - seg[0] > min_duration]


def _plot_segments(signal, sampling_rate, prob, st_step, seg_limits):
    # waveform and probability curve with the segment limits marked (:793-811)
    import matplotlib.pyplot as plt
    curves = ((np.arange(signal.shape[0]) / float(sampling_rate), signal, 'Signal'),
              (np.arange(prob.shape[0]) * st_step, prob, 'svm Probability'))
    for row, (xs, ys, title) in enumerate(curves):
        plt.subplot(2, 1, row + 1)
        plt.plot(xs, ys)
        for lo, hi in seg_limits:
            plt.axvline(x=lo, color='red')
            plt.axvline(x=hi, color='red')
        plt.title(title)
    plt.show()


def _train_onset_svm_device(low_energy, high_energy, random_state, kernel_cache="none", cache_bytes=None):
    """_train_onset_svm without scikit-learn: StandardScaler's mean_ / scale_ (a constant feature keeps scale 1), applied on the
    load path of audioTrainTest.train_svm_device's fits (C = 1, linear, gamma='auto', probability=True)."""
    from . import audioTrainTest as aT
    features = np.vstack([low_energy, high_energy])
    labels = np.append(np.zeros(low_energy.shape[0]), np.ones(high_energy.shape[0]))
    mean = features.mean(axis=0)
    scale = np.sqrt(features.var(axis=0))
    scale[scale < 10 * np.finfo(np.float64).eps] = 1.0                                     # sklearn's _handle_zeros_in_scale
    cache = () if kernel_cache == "none" else (kernel_cache, cache_bytes)
    return aT._train_svm_device(features, labels, 1.0, 'linear', random_state, mean, scale, *cache), mean, scale


def silence_removal(signal, sampling_rate, st_win, st_step, smooth_window=0.5, weight=0.5, plot=False, *, svm_fit="sklearn",
                    random_state=None, kernel_cache="none", cache_bytes=None):
    """Event detection (silence removal), reference :672-815.  Returns the list of [start, end] segments in seconds.

    signal, sampling_rate: the audio; st_win, st_step: short-term window and step in SECONDS; smooth_window: length of
    the probability smoothing in seconds; weight in (0, 1): the higher, the stricter (values outside are pulled to
    0.01 / 0.99, :697-700).  svm_fit (keyword only): "sklearn" (the default) trains the onset SVM with scikit-learn; "device"
    trains it on the GPU (audioTrainTest.train_svm_device: the full fit, libsvm's five cross-validation fits and the sigmoid
    fit) and needs no scikit-learn; random_state is read by that mode alone (None: one draw from NumPy's global state, as
    scikit-learn's fit makes).  Any other value of svm_fit raises ValueError.  kernel_cache / cache_bytes (keyword only, read
    under svm_fit="device"; anything but their defaults raises ValueError otherwise) are audioTrainTest.train_svm_device's:
    under "gram" the full fit and the five fold fits read one resident kernel matrix, with the same segments."""
    if svm_fit not in ("sklearn", "device"):
        raise ValueError("svm_fit=%r: 'sklearn' or 'device'" % (svm_fit,))
    from . import audioTrainTest as aT
    aT._svc_cache_mode(kernel_cache, cache_bytes, svm_fit == "device", "svm_fit")
    from . import ShortTermFeatures as stf
    weight = min(max(weight, 0.01), 0.99) if not 0 < weight < 1 else weight
    mono = audioBasicIO.stereo_to_mono(signal)
    st_feats, _ = stf.feature_extraction(mono, sampling_rate, st_win * sampling_rate, st_step * sampling_rate)   # :707-710
    quiet, loud = _energy_extremes(st_feats)
    if svm_fit == "device":
        cache = () if kernel_cache == "none" else (kernel_cache, cache_bytes)
        svm, mean, std = _train_onset_svm_device(quiet.T, loud.T, random_state, *cache)
    else:
        svm, mean, std = _train_onset_svm(quiet.T, loud.T)                                 # :730-739, scikit-learn
    # onset probability of every frame in one kernel (replaces the predict_proba loop :741-748), then smoothing (:751)
    prob = smooth_moving_avg(svm_onset_probability(st_feats, mean, std, svm), smooth_window / st_step)
    active = np.flatnonzero(prob > _onset_threshold(prob, weight))                         # :761
    seg_limits = _onset_segments(active, st_step)
    if plot:
        _plot_segments(mono, sampling_rate, prob, st_step, seg_limits)
    return seg_limits


# ---------------------------------------------------------------------------------------------------------
# silence removal of many clips in one call (kernels_onset.hpp, lib_onset.hpp)
# ---------------------------------------------------------------------------------------------------------
ONSET_MIN_FRAMES = 20      # int(T / 10) >= 2: the reference's ranked[-tenth:-1] is not empty


def _per_clip(value, n, name):
    """a scalar or one value per clip -> float64 [n]"""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        return np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError("%s: a scalar or one value per clip (%d clips, shape %s)" % (name, n, a.shape))
    return np.ascontiguousarray(a)


def _batch_seeds(random_state, n):
    """libsvm's random_seed of n fits, one draw each in clip order: None draws from NumPy's global state exactly as
    audioTrainTest._libsvm_seed does in n calls, an int makes ONE RandomState that is drawn from n times, a RandomState is
    used as is."""
    from . import audioTrainTest as aT
    if random_state is None:
        return [aT._libsvm_seed(None) for _ in range(n)]
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    return [aT._libsvm_seed(rs) for _ in range(n)]


def _onset_plan(lengths, sampling_rate, st_win, st_step, smooth_window, weight):
    """The argument half of silence_removal_batch, without the device: (window, step, frames, widths, weights) or the
    ValueError of the first clip that cannot be served."""
    n = len(lengths)
    window, step = int(st_win * sampling_rate), int(st_step * sampling_rate)      # ShortTermFeatures.py:563-564
    if window < 2 or step < 1:
        raise ValueError("st_win = %r, st_step = %r at %r Hz: a window of %d and a step of %d samples" % (st_win, st_step, sampling_rate, window, step))
    smooth = _per_clip(smooth_window, n, "smooth_window")
    weights = _per_clip(weight, n, "weight")
    weights = np.where((weights > 0) & (weights < 1), weights, np.minimum(np.maximum(weights, 0.01), 0.99))   # :697-700
    frames = np.array([(int(m) - window) // step + 1 if int(m) >= window else 0 for m in lengths], dtype=np.int64)
    widths = np.array([int(s / st_step) for s in smooth], dtype=np.int32)          # smooth_moving_avg's int(window)
    for c in range(n):
        if frames[c] < ONSET_MIN_FRAMES:
            raise ValueError("clip %d: %d short-term frames: at least %d are needed (the mean of the loudest tenth leaves its "
                             "maximum out)" % (c, frames[c], ONSET_MIN_FRAMES))
        if frames[c] < widths[c]:
            raise ValueError("clip %d: Input vector needs to be bigger than window size. (%d frames, a smoothing window of %d)"
                             % (c, frames[c], widths[c]))
    return window, step, frames, widths, np.ascontiguousarray(weights, dtype=np.float64)


def _silence_group(clips, as_i16, sampling_rate, window, step, frames, widths, weights, seeds, chunk_bytes, stage_ms, cache_bytes=None):
    """The call of paa_silence_batch_* for clips of one sample type; returns the per-clip detail records.  The library's refusals
    after the selection (an empty set: ValueError; more than 8192 rows: NotImplementedError) name the clip themselves.
    cache_bytes (None: no resident kernel matrices) selects paa_silence_batch_*_cached; a record's `cached` tells whether the
    clip's fits read one."""
    from . import audioTrainTest as aT
    n, D = len(clips), 68
    lens = np.array([c.shape[0] for c in clips], dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    packed = np.concatenate(clips) if n > 1 else clips[0]
    frame_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(frames, out=frame_off[1:])
    cap_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.minimum(2 * frames, aT.SMO_MAX_ROWS), out=cap_off[1:])
    nf, nr = int(frame_off[-1]), int(cap_off[-1])
    quiet, loud, active = (np.zeros(nf, dtype=np.uint8) for _ in range(3))
    raw, prob = np.zeros(nf), np.zeros(nf)
    limits, counts = np.zeros((n, 2)), np.zeros((n, 2), dtype=np.int32)
    mean, scale = np.zeros((n, D)), np.zeros((n, D))
    src, alpha_y = np.zeros(nr, dtype=np.int32), np.zeros(nr)
    rho, prob_a, prob_b, thr = (np.zeros(n) for _ in range(4))
    n_sv, sig_it, sig_stop = (np.zeros(n, dtype=np.int32) for _ in range(3))
    iterations, status = np.zeros((n, 6), dtype=np.int32), np.zeros((n, 6), dtype=np.int32)
    seed = np.ascontiguousarray(seeds, dtype=np.int64)
    lib = _ffi.lib()
    cached = np.zeros(n, dtype=np.int32)
    if cache_bytes is None:
        fn, tail = lib.paa_silence_batch_i16 if as_i16 else lib.paa_silence_batch_f64, ()
    else:
        fn, tail = lib.paa_silence_batch_i16_cached if as_i16 else lib.paa_silence_batch_f64_cached, (int(cache_bytes), _ffi.as_i32p(cached))
    rc = fn(_ffi.as_i16p(packed) if as_i16 else _ffi.as_f64p(packed), _ffi.as_i64p(offsets), n, float(sampling_rate), window, step,
            _ffi.as_i32p(widths), _ffi.as_f64p(weights), _ffi.as_i64p(seed), int(chunk_bytes or 0), _ffi.as_i64p(cap_off),
            _ffi.as_u8p(quiet), _ffi.as_u8p(loud), _ffi.as_u8p(active), _ffi.as_f64p(raw), _ffi.as_f64p(prob), _ffi.as_f64p(limits),
            _ffi.as_i32p(counts), _ffi.as_f64p(mean), _ffi.as_f64p(scale), _ffi.as_i32p(src), _ffi.as_f64p(alpha_y), _ffi.as_f64p(rho),
            _ffi.as_f64p(prob_a), _ffi.as_f64p(prob_b), _ffi.as_f64p(thr), _ffi.as_i32p(n_sv), _ffi.as_i32p(iterations),
            _ffi.as_i32p(status), _ffi.as_i32p(sig_it), _ffi.as_i32p(sig_stop), _ffi.as_f64p(stage_ms) if stage_ms is not None else None,
            *tail)
    _ffi.check(rc)
    aT._warn_not_converged(status.reshape(-1), 10 ** 7)
    out = []
    for c in range(n):
        f0, f1, r0 = int(frame_off[c]), int(frame_off[c + 1]), int(cap_off[c])
        nq, nl = int(counts[c, 0]), int(counts[c, 1])
        out.append(dict(quiet_idx=src[r0:r0 + nq].astype(np.int64), loud_idx=src[r0 + nq:r0 + nq + nl].astype(np.int64),
                        quiet_limit=float(limits[c, 0]), loud_limit=float(limits[c, 1]), mean=mean[c].copy(), scale=scale[c].copy(),
                        seed=int(seed[c]), alpha_y=alpha_y[r0:r0 + nq + nl].copy(), rho=float(rho[c]), prob_a=float(prob_a[c]),
                        prob_b=float(prob_b[c]), n_sv=int(n_sv[c]), status=status[c].copy(), iterations=iterations[c].copy(),
                        sigmoid_iterations=int(sig_it[c]), sigmoid_stop=int(sig_stop[c]), raw_prob=raw[f0:f1].copy(),
                        prob=prob[f0:f1].copy(), threshold=float(thr[c]), active=np.flatnonzero(active[f0:f1]), cached=bool(cached[c])))
    return out


def _silence_batch(signals, sampling_rate, st_win, st_step, smooth_window, weight, seeds, chunk_bytes, stage_ms=None, cache_bytes=None):
    """silence_removal_batch with the seeds given (a callable that draws them once the arguments have passed).  The whole batch is
    ONE library call, so that every refusal that follows the selection comes before any fit: int16 clips travel as int16; if
    any clip has another dtype the whole batch goes through np.double (feature_extraction_batch's rule).  Returns the per-clip
    detail records in clip order."""
    monos = [np.asarray(audioBasicIO.stereo_to_mono(s)) for s in signals]
    for c, m in enumerate(monos):
        if m.ndim != 1:
            raise ValueError("clip %d: a signal of %d dimensions (mono, or two channels)" % (c, m.ndim))
    window, step, frames, widths, weights = _onset_plan([m.shape[0] for m in monos], sampling_rate, st_win, st_step, smooth_window, weight)
    seeds = seeds(len(monos)) if callable(seeds) else list(seeds)
    as_i16 = all(m.dtype == np.int16 for m in monos)
    clips = [np.ascontiguousarray(m if as_i16 else np.double(m)) for m in monos]
    cache = () if cache_bytes is None else (cache_bytes,)
    return _silence_group(clips, as_i16, sampling_rate, window, step, frames, widths, weights, seeds, chunk_bytes, stage_ms, *cache)


def silence_removal_batch(signals, sampling_rate, st_win, st_step, smooth_window=0.5, weight=0.5, *, random_state=None,
                          return_details=False, chunk_bytes=None, kernel_cache="none", cache_bytes=None):
    """silence_removal(.., svm_fit="device") for a list of clips of ONE sampling rate, on the GPU end to end: the short-term
    matrices of the batched plan stay in device memory, and energy selection, training sets with their scalers, the SVM fits
    of all clips (one solver batch), the per-frame probabilities, smoothing and thresholds are kernels over the whole batch.
    Returns one list of [start, end] segments in seconds per clip, as silence_removal gives them; scikit-learn is not needed.

    signals: the clips (each through audioBasicIO.stereo_to_mono); st_win, st_step in seconds, one pair per call;
    smooth_window and weight: a scalar, or one value per clip (weight is pulled into 0.01 .. 0.99 as in the single call).
    random_state: None draws one seed per clip from NumPy's global state -- clip i sees the seed that the i-th call of a loop
    of silence_removal(.., svm_fit="device") would see; an int makes ONE RandomState(int) that is drawn from once per clip; a
    RandomState is used as is.  The seeds are drawn on the host in clip order before any device work, after the arguments
    have passed.  int16 clips travel as int16; if any clip has another dtype the whole batch goes through np.double.  return_details=True returns (segments, details): per clip a dict of quiet_idx, loud_idx, quiet_limit,
    loud_limit, mean, scale, seed, alpha_y (over the quiet rows, then the loud rows), rho, prob_a, prob_b, n_sv, status and
    iterations [6] (the full fit, the five folds), sigmoid_iterations, sigmoid_stop, raw_prob, prob (smoothed), threshold and
    active.  chunk_bytes: a bound below the library's 1 GiB for the device scratch of one chunk of clips (tests); no result
    depends on it.  kernel_cache / cache_bytes (keyword only) are audioTrainTest.svc_fit_proba's with the clip as the job: under
    "gram" a clip's full fit and fold fits read one resident kernel matrix (paa_silence_batch_*_cached), every result is
    byte-equal, and the details carry `cached`.

    ValueError names the clip: fewer than 20 frames, or fewer than int(smooth_window / st_step) (both before the device is
    touched); an empty quiet or loud set (after the selection, before any fit).  NotImplementedError for a clip whose quiet
    and loud rows exceed the solver's 8192."""
    from . import audioTrainTest as aT
    cache_bytes = aT._cache_mode(kernel_cache, cache_bytes)
    signals = list(signals)
    if not signals:
        return ([], []) if return_details else []
    details = _silence_batch(signals, sampling_rate, st_win, st_step, smooth_window, weight,
                             lambda n: _batch_seeds(random_state, n), chunk_bytes, cache_bytes=cache_bytes)
    segments = [_onset_segments(d["active"], st_step) for d in details]
    return (segments, details) if return_details else segments


def _as_path_index(exc, ids):
    """the refusal of clip k of a group, renamed to the path it came from"""
    msg = str(exc)
    if not msg.startswith("clip "):
        return exc
    head, _, rest = msg.partition(":")
    return type(exc)("clip %d:%s" % (ids[int(head[5:])], rest))


def silence_removal_files(paths, st_win, st_step, smooth_window=0.5, weight=0.5, *, random_state=None, kernel_cache="none",
                          cache_bytes=None):
    """silence_removal_batch over audio files: they are read and grouped by sampling rate, one device batch per rate; the
    seeds are drawn in path order and the segment lists come back in path order.  smooth_window and weight: a scalar or one
    value per path.  A file that cannot be read raises ValueError naming its index.  As in silence_removal_batch the arguments
    of EVERY file are checked before a seed is drawn or the device is touched; a refusal that follows the selection comes before
    the fits of its own rate's batch (the batches of other rates may have run).  kernel_cache / cache_bytes (keyword only) are
    silence_removal_batch's."""
    from . import audioTrainTest as aT
    cache_bytes = aT._cache_mode(kernel_cache, cache_bytes)
    paths = list(paths)
    n = len(paths)
    smooth, weights = _per_clip(smooth_window, n, "smooth_window"), _per_clip(weight, n, "weight")
    groups = {}
    for i, path in enumerate(paths):
        fs, sig = audioBasicIO.read_audio_file(path)
        if fs <= 0:
            raise ValueError("file %d (%s) cannot be read" % (i, path))
        groups.setdefault(fs, []).append((i, np.asarray(audioBasicIO.stereo_to_mono(sig))))
    for fs, members in groups.items():
        ids = [i for i, _ in members]
        try:
            _onset_plan([s.shape[0] for _, s in members], fs, st_win, st_step, smooth[ids], weights[ids])
        except ValueError as exc:
            raise _as_path_index(exc, ids)
    seeds = _batch_seeds(random_state, n)
    out = [None] * n
    for fs, members in groups.items():
        ids = [i for i, _ in members]
        try:
            details = _silence_batch([s for _, s in members], fs, st_win, st_step, smooth[ids], weights[ids], [seeds[i] for i in ids], None,
                                     cache_bytes=cache_bytes)
        except (ValueError, NotImplementedError) as exc:
            raise _as_path_index(exc, ids)
        for i, d in zip(ids, details):
            out[i] = _onset_segments(d["active"], st_step)
    return out


def _stack_matrices(st_feats_list):
    """list of (n_dims x T_c) matrices -> (packed float64, frames int32 [n], n_dims)"""
    mats = [np.ascontiguousarray(np.asarray(f, dtype=np.float64)) for f in st_feats_list]
    if not mats:
        raise ValueError("need at least one short-term matrix")
    if any(m.ndim != 2 for m in mats) or any(m.shape[0] != mats[0].shape[0] for m in mats):
        raise ValueError("the short-term matrices must be (n_dims x frames) with one n_dims")
    frames = np.array([m.shape[1] for m in mats], dtype=np.int32)
    for c, t in enumerate(frames):
        if t < ONSET_MIN_FRAMES:
            raise ValueError("clip %d: %d short-term frames: at least %d are needed" % (c, t, ONSET_MIN_FRAMES))
    packed = np.concatenate([m.reshape(-1) for m in mats]) if len(mats) > 1 else mats[0].reshape(-1)
    return packed, frames, mats[0].shape[0]


def onset_training_sets(st_feats_list, *, chunk_bytes=None):
    """Stages 1 and 2 of silence_removal_batch for short-term matrices in host memory (onset_select_kernel,
    onset_gather_kernel): per clip a dict of quiet_limit, loud_limit, quiet_idx, loud_idx (frames with energy <= / >= the
    limit; a frame may be in both), features (np.vstack([quiet.T, loud.T]) of _energy_extremes), mean and scale (NumPy's
    features.mean(axis=0) and sqrt(var(axis=0)) bit for bit, a scale below 10 eps set to 1).  An empty set is reported, not
    refused (silence_removal_batch raises for it)."""
    packed, frames, D = _stack_matrices(st_feats_list)
    n, nf = len(frames), int(frames.sum())
    cap = 2 * nf
    limits, counts = np.zeros((n, 2)), np.zeros((n, 2), dtype=np.int32)
    quiet, loud = np.zeros(nf, dtype=np.uint8), np.zeros(nf, dtype=np.uint8)
    src, X = np.zeros(cap, dtype=np.int32), _ffi.result_array((cap, D))
    mean, scale = np.zeros((n, D)), np.zeros((n, D))
    _ffi.check(_ffi.lib().paa_onset_training_sets_f64(
        _ffi.as_f64p(packed), _ffi.as_i32p(frames), n, D, int(chunk_bytes or 0), cap, _ffi.as_f64p(limits), _ffi.as_i32p(counts),
        _ffi.as_u8p(quiet), _ffi.as_u8p(loud), _ffi.as_i32p(src), _ffi.as_f64p(X), _ffi.as_f64p(mean), _ffi.as_f64p(scale)))
    out, r0, f0 = [], 0, 0
    for c in range(n):
        nq, nl = int(counts[c, 0]), int(counts[c, 1])
        out.append(dict(quiet_limit=float(limits[c, 0]), loud_limit=float(limits[c, 1]), quiet_idx=src[r0:r0 + nq].astype(np.int64),
                        loud_idx=src[r0 + nq:r0 + nq + nl].astype(np.int64), features=X[r0:r0 + nq + nl].copy(), mean=mean[c].copy(),
                        scale=scale[c].copy(), quiet_flags=quiet[f0:f0 + frames[c]].astype(bool), loud_flags=loud[f0:f0 + frames[c]].astype(bool)))
        r0 += nq + nl
        f0 += int(frames[c])
    return out


def onset_activity(st_feats_list, models, widths, weights, *, chunk_bytes=None):
    """Stages 4 and 5 of silence_removal_batch for short-term matrices in host memory and one linear model per clip
    (onset_proba_kernel, onset_threshold_kernel).  models: per clip (w, intercept, prob_a, prob_b, mean, scale) -- scikit-learn's
    decision_function is <w, (x - mean) / scale> + intercept; widths: the smoothing box in frames (int(smooth_window /
    st_step)), weights: the threshold weight, each a scalar or one per clip.  Per clip a dict of raw_prob, prob (smoothed),
    threshold and active (the frames with prob > threshold)."""
    packed, frames, D = _stack_matrices(st_feats_list)
    n, nf = len(frames), int(frames.sum())
    models = list(models)
    if len(models) != n or any(len(m) != 6 for m in models):
        raise ValueError("one model (w, intercept, prob_a, prob_b, mean, scale) per clip")
    vec = lambda k: np.ascontiguousarray(np.stack([np.asarray(m[k], dtype=np.float64).reshape(-1) for m in models]))
    w, mean, scale = vec(0), vec(4), vec(5)
    if w.shape != (n, D) or mean.shape != (n, D) or scale.shape != (n, D):
        raise ValueError("feature dimension mismatch between the matrices and the models")
    icpt, pa, pb = (np.array([float(m[k]) for m in models]) for k in (1, 2, 3))
    wd = np.ascontiguousarray(_per_clip(widths, n, "widths").astype(np.int32))
    wt = _per_clip(weights, n, "weights")
    for c in range(n):
        if frames[c] < wd[c]:
            raise ValueError("clip %d: Input vector needs to be bigger than window size." % c)
    raw, prob, thr, active = np.zeros(nf), np.zeros(nf), np.zeros(n), np.zeros(nf, dtype=np.uint8)
    _ffi.check(_ffi.lib().paa_onset_activity_f64(
        _ffi.as_f64p(packed), _ffi.as_i32p(frames), n, D, _ffi.as_f64p(w), _ffi.as_f64p(icpt), _ffi.as_f64p(pa), _ffi.as_f64p(pb),
        _ffi.as_f64p(mean), _ffi.as_f64p(scale), _ffi.as_i32p(wd), _ffi.as_f64p(wt), int(chunk_bytes or 0), _ffi.as_f64p(raw),
        _ffi.as_f64p(prob), _ffi.as_f64p(thr), _ffi.as_u8p(active)))
    out, f0 = [], 0
    for c in range(n):
        f1 = f0 + int(frames[c])
        out.append(dict(raw_prob=raw[f0:f1].copy(), prob=prob[f0:f1].copy(), threshold=float(thr[c]), active=np.flatnonzero(active[f0:f1])))
        f0 = f1
    return out


# ---------------------------------------------------------------------------------------------------------
# fix-sized segment classification with the SVM, kNN and tree-ensemble models (reference :58-125, :150-175, :495-633)
# ---------------------------------------------------------------------------------------------------------
def labels_to_segments(labels, window):
    """Fix-sized class labels -> (segments [n][2] of start / end in seconds, class of each segment) (reference :58-98)."""
    if len(labels) == 1:
        segs = [0, window]
        classes = labels
        return segs, classes
    num_segs = 0
    index = 0
    classes = []
    segment_list = []
    cur_label = labels[index]
    while index < len(labels) - 1:
        previous_value = cur_label
        while True:
            index += 1
            compare_flag = labels[index]
            if (compare_flag != cur_label) | (index == len(labels) - 1):
                num_segs += 1
                cur_label = labels[index]
                segment_list.append((index * window))
                classes.append(previous_value)
                break
    segments = np.zeros((len(segment_list), 2))
    for i in range(len(segment_list)):
        if i > 0:
            segments[i, 0] = segment_list[i - 1]
        segments[i, 1] = segment_list[i]
    return segments, classes


def segments_to_labels(start_times, end_times, labels, window):
    """Segment end points and labels -> (fix-sized class indices, class names) (reference :101-125).  The class names
    come from list(set(labels)), so their order follows Python's string hashing, as in the reference."""
    flags = []
    class_names = list(set(labels))
    index = window / 2.0
    while index < end_times[-1]:
        for i in range(len(start_times)):
            if start_times[i] < index <= end_times[i]:
                break
        flags.append(class_names.index(labels[i]))
        index += window
    return np.array(flags), class_names


def read_segmentation_gt(gt_file):
    """<start>\\t<end>\\t<label> rows of a ground-truth file -> (starts, ends, labels) (reference :150-175)."""
    import csv
    with open(gt_file, 'rt') as f_handle:
        reader = csv.reader(f_handle, delimiter='\t')
        start_times = []
        end_times = []
        labels = []
        for row in reader:
            if len(row) == 3:
                start_times.append(float(row[0]))
                end_times.append(float(row[1]))
                labels.append((row[2]))
    return np.array(start_times), np.array(end_times), labels


def plot_segmentation_results(flags_ind, flags_ind_gt, class_names, mt_step, evaluate_only=False):
    """Accuracy of fix-sized labels against the ground truth (reference :178-247); the per-class statistics and the
    matplotlib figure only when evaluate_only is False."""
    flags = [class_names[int(f)] for f in flags_ind]
    segments, classes = labels_to_segments(flags, mt_step)
    min_len = min(flags_ind.shape[0], flags_ind_gt.shape[0])
    if min_len > 0:
        accuracy = np.sum(flags_ind[0:min_len] == flags_ind_gt[0:min_len]) / float(min_len)
    else:
        accuracy = -1
    if not evaluate_only:
        import matplotlib.pyplot as plt
        duration = segments[-1, 1]
        s_percentages = np.zeros((len(class_names), ))
        percentages = np.zeros((len(class_names), ))
        av_durations = np.zeros((len(class_names), ))
        for i_seg in range(segments.shape[0]):
            s_percentages[class_names.index(classes[i_seg])] += (segments[i_seg, 1] - segments[i_seg, 0])
        for i in range(s_percentages.shape[0]):
            percentages[i] = 100.0 * s_percentages[i] / duration
            class_sum = sum(1 for c in classes if c == class_names[i])
            av_durations[i] = s_percentages[i] / class_sum if class_sum > 0 else 0.0
        for i in range(percentages.shape[0]):
            print(class_names[i], percentages[i], av_durations[i])
        fig = plt.figure()
        ax1 = fig.add_subplot(211)
        ax1.set_yticks(np.array(range(len(class_names))))
        ax1.axis((0, duration, -1, len(class_names)))
        ax1.set_yticklabels(class_names)
        ax1.plot(np.array(range(len(flags_ind))) * mt_step + mt_step / 2.0, flags_ind)
        if flags_ind_gt.shape[0] > 0:
            ax1.plot(np.array(range(len(flags_ind_gt))) * mt_step + mt_step / 2.0, flags_ind_gt + 0.05, '--r')
        plt.xlabel("time (seconds)")
        if accuracy >= 0:
            plt.title('Accuracy = {0:.1f}%'.format(100.0 * accuracy))
        ax2 = fig.add_subplot(223)
        plt.title("Classes percentage durations")
        ax2.bar(np.array(range(len(class_names))) + 0.5, percentages)
        ax3 = fig.add_subplot(224)
        plt.title("Segment average duration per class")
        ax3.bar(np.array(range(len(class_names))) + 0.5, av_durations)
        fig.tight_layout()
        plt.show()
    return accuracy


def load_ground_truth_segments(gt_file, mt_step):
    """Reference :495-508."""
    seg_start, seg_end, seg_labels = read_segmentation_gt(gt_file)
    labels, class_names = segments_to_labels(seg_start, seg_end, seg_labels, mt_step)
    labels_temp = []
    for index, label in enumerate(labels):
        if class_names[labels[index]] in class_names:
            labels_temp.append(class_names.index(class_names[labels[index]]))
        else:
            labels_temp.append(-1)
    return np.array(labels_temp), class_names


def calculate_confusion_matrix(predictions, ground_truth, classes):
    """Reference :511-516: rows ground truth, columns predictions."""
    cm = np.zeros((len(classes), len(classes)))
    for index in range(min(predictions.shape[0], ground_truth.shape[0])):
        cm[int(ground_truth[index]), int(predictions[index])] += 1
    return cm


def load_ground_truth(gt_file, labels, class_names, mid_step, plot_results):
    """Reference :606-633: (ground-truth labels, class names, accuracy, confusion matrix) when gt_file exists."""
    import os
    accuracy = 0
    cm = np.array([])
    labels_gt = np.array([])
    if os.path.isfile(gt_file):
        labels_gt, class_names_gt = load_ground_truth_segments(gt_file, mid_step)
        labels_new = []
        for il, l in enumerate(labels):
            if class_names[int(l)] in class_names_gt:
                labels_new.append(class_names_gt.index(class_names[int(l)]))
            else:
                labels_new.append(-1)
        labels_new = np.array(labels_new)
        cm = calculate_confusion_matrix(labels_new, labels_gt, class_names_gt)
        accuracy = plot_segmentation_results(labels_new, labels_gt, class_names_gt, mid_step, not plot_results)
        if accuracy >= 0:
            print("Overall Accuracy: {0:.2f}".format(accuracy))
    return labels_gt, class_names, accuracy, cm


def _mid_term_on_device(signal, sampling_rate, mid_window, mid_step, st_window_samples, st_step_samples, extra_rows=0):
    """A context manager that yields (d_mid, M): the mid-term matrix of a mono signal left in HBM, a DeviceBuffer of
    [136 + extra_rows][M] doubles whose first 136 rows are the features of the M mid-term windows.  The arguments are
    tested at this call (every ValueError precedes any device work); the plan and the buffers are made when the with
    block is entered and freed when it is left, whatever happened.  The short-term window and step come in samples, as
    the caller rounds them."""
    from . import MidTermFeatures
    ratio, step_ratio = MidTermFeatures._ratios(mid_window * sampling_rate, mid_step * sampling_rate, st_window_samples,
                                                st_step_samples)
    if step_ratio < 1:
        raise ValueError("mid_step / short_step rounds to 0: the reference never terminates")
    window, step = int(st_window_samples), int(st_step_samples)
    kind, sig = _ffi.classify_signal(signal)
    if kind == 2:
        raise ValueError("mono signal expected (audioBasicIO.stereo_to_mono first)")
    n = sig.shape[0]
    if window < 1 or step < 1 or n < window:
        raise ValueError("need at least one array to concatenate")          # ShortTermFeatures.py:684

    @contextlib.contextmanager
    def on_device():
        plan = _ffi.Plan(np.array([0, n], dtype=np.int64), sampling_rate, window, step, deltas=True, sample_kind=kind)
        bufs = []
        try:
            bufs.append(_ffi.DeviceBuffer.from_host(sig))
            bufs.append(_ffi.DeviceBuffer(plan.out_doubles * 8))
            plan.execute(bufs[0], bufs[1])
            n_mid = plan.mid_doubles(step_ratio)
            M = n_mid // (2 * 68)
            bufs.append(_ffi.DeviceBuffer((n_mid + extra_rows * M) * 8))
            plan.mid_execute(bufs[1], ratio, step_ratio, bufs[2])
            yield bufs[2], M
        finally:
            for b in bufs:
                b.free()
            plan.destroy()
    return on_device()


def mid_term_labels(signal, sampling_rate, classifier, mean, std, mt_win, mid_step, st_win, st_step, model_type=None):
    """Labels and max-probabilities of every mid-term window of a mono signal (reference :574-594): the mid-term matrix
    stays in HBM and goes straight into the SVC, kNN or tree-ensemble kernels (one launch for all windows).  Returns
    (labels, posterior max): an SVM's or tree ensemble's classes_, a kNN model's class indices.  model_type "knn", a
    tree-ensemble type or an SVM type; None takes the model's kind (audioTrainTest.is_knn / is_forest)."""
    from . import audioTrainTest
    mid = _mid_term_on_device(signal, sampling_rate, mt_win, mid_step, round(sampling_rate * st_win), round(sampling_rate * st_step))
    model = audioTrainTest.device_model(classifier, model_type)
    with mid as (d_mid, M):
        idx, proba = model.predict_device(d_mid, M, M, mean, std)
    return model.labels(idx), np.max(proba, axis=1)


def mid_term_regression_signal(signal, sampling_rate, models, means, stds, model_type, mt_win, mid_step, st_win, st_step):
    """The regression values of every mid-term window of a mono signal -- a target such as arousal along a recording:
    [n_models][n_windows].  An addition without a counterpart in the reference (which regresses whole files only,
    audioTrainTest.file_regression): the mid-term matrix stays in HBM and goes straight into the SVR bank kernel (one
    launch for all models and windows) or, for "randomforest", into one traversal / reduction pair per forest.  means /
    stds: one row per model, or one vector shared by all."""
    from . import audioTrainTest
    if model_type not in audioTrainTest._REGRESSION_TYPES:
        raise NotImplementedError("regression model type %r: the GPU path serves 'svm', 'svm_rbf' and 'randomforest'" % (model_type,))
    mid = _mid_term_on_device(signal, sampling_rate, mt_win, mid_step, round(sampling_rate * st_win), round(sampling_rate * st_step))
    if model_type in audioTrainTest._SVM_TYPES:
        bank = audioTrainTest.svr_bank(models, means, stds)
        with mid as (d_mid, M):
            return bank.predict_device(d_mid, M, M)
    forests = [audioTrainTest._forest_regressor(m) for m in models]
    means = audioTrainTest._stats_rows(means, len(forests), forests[0].n_dims, "means")
    stds = audioTrainTest._stats_rows(stds, len(forests), forests[0].n_dims, "stds")
    with mid as (d_mid, M):
        return np.stack([f.predict_device(d_mid, M, M, means[i], stds[i])[1][:, 0] for i, f in enumerate(forests)])


def mid_term_classification(signal, sampling_rate, classifier, mean, std, class_names, mt_win, mid_step, st_win, st_step,
                            compute_beat=False, plot_results=False, gt_file="", model_type=None):
    """mid_term_file_classification on a signal and a loaded SVM, kNN or tree-ensemble model (reference :518-604 from
    :562 on):
    returns (labels, class_names, accuracy, cm)."""
    labels = []
    accuracy = 0.0
    cm = np.array([])
    if compute_beat:
        print("Model contains long-term music features (beat etc) and cannot be used in segmentation")
        return labels, class_names, accuracy, cm
    signal = audioBasicIO.stereo_to_mono(signal)
    labels, _ = mid_term_labels(signal, sampling_rate, classifier, mean, std, mt_win, mid_step, st_win, st_step,
                                model_type)
    segs, classes = labels_to_segments(labels, mid_step)
    for i in range(len(segs)):
        print(segs[i], classes[i])
    segs[-1] = len(signal) / float(sampling_rate)
    labels_gt, class_names_gt, accuracy, cm = load_ground_truth(gt_file, labels, class_names, mid_step, plot_results)
    return labels, class_names, accuracy, cm


def mid_term_file_classification(input_file, model_name, model_type, plot_results=False, gt_file=""):
    """Mid-term classification of an audio file with a trained SVM, kNN or tree-ensemble model (reference :518-604): returns
    (labels, class_names, accuracy, cm).  Models with compute_beat are refused, as in the reference."""
    import os
    from . import audioTrainTest
    labels = []
    accuracy = 0.0
    class_names = []
    cm = np.array([])
    if not os.path.isfile(model_name):
        print("mtFileClassificationError: input model_type not found!")
        return labels, class_names, accuracy, cm
    if model_type not in ("svm", "svm_rbf", "knn") + audioTrainTest._FOREST_TYPES:
        raise NotImplementedError("model type %r: the GPU path serves the SVM, kNN and tree-ensemble models" % (model_type,))
    classifier, mean, std, class_names, mt_win, mid_step, st_win, st_step, compute_beat = audioTrainTest._load(model_name, model_type)
    if compute_beat:
        print("Model " + model_name + " contains long-term music features (beat etc) and cannot be used in segmentation")
        return labels, class_names, accuracy, cm
    sampling_rate, signal = audioBasicIO.read_audio_file(input_file)
    if sampling_rate == 0:
        return labels, class_names, accuracy, cm
    return mid_term_classification(signal, sampling_rate, classifier, mean, std, class_names, mt_win, mid_step, st_win,
                                   st_step, False, plot_results, gt_file, model_type)


# ---------------------------------------------------------------------------------------------------------
# joint segmentation-classification with a Gaussian HMM (reference :287-492)
# ---------------------------------------------------------------------------------------------------------
def _release_hmm(handle):
    _ffi.lib().paa_hmm_destroy(handle)


class GaussianHmm:
    """A Gaussian HMM with one diagonal Gaussian per state, with the attributes the reference sets on hmmlearn's
    GaussianHMM (startprob_, transmat_, means_, covars_ -- the latter holds what the reference puts there, the per-class
    standard deviation, :340).  predict / decode are hmmlearn's (Viterbi, lowest index among equal maxima) on the GPU;
    the model is uploaded at the first call (ValueError when paa_hmm_create refuses it) and freed with the object."""
    covariance_type = "diag"

    def __init__(self, startprob, transmat, means, covars):
        self.startprob_ = np.ascontiguousarray(np.asarray(startprob, dtype=np.float64).reshape(-1))
        self.means_ = np.ascontiguousarray(np.atleast_2d(np.asarray(means, dtype=np.float64)))
        self.covars_ = np.ascontiguousarray(np.atleast_2d(np.asarray(covars, dtype=np.float64)))
        self.n_components = self.startprob_.shape[0]
        self.transmat_ = np.ascontiguousarray(np.asarray(transmat, dtype=np.float64).reshape(self.n_components, -1))
        k = self.n_components
        if self.transmat_.shape != (k, k) or self.means_.shape[0] != k or self.covars_.shape != self.means_.shape:
            raise ValueError("HMM arrays disagree: startprob %s, transmat %s, means %s, covars %s"
                             % (self.startprob_.shape, self.transmat_.shape, self.means_.shape, self.covars_.shape))
        self.n_features = self.means_.shape[1]
        self._handle = None

    def __getstate__(self):
        return {"startprob_": self.startprob_, "transmat_": self.transmat_, "means_": self.means_, "covars_": self.covars_}

    def __setstate__(self, state):
        self.__init__(state["startprob_"], state["transmat_"], state["means_"], state["covars_"])

    @property
    def handle(self):
        if self._handle is None:
            import weakref
            lib = _ffi.lib()
            handle = C.c_void_p()
            rc = lib.paa_hmm_create(_ffi.as_f64p(self.startprob_), _ffi.as_f64p(self.transmat_), _ffi.as_f64p(self.means_),
                                    _ffi.as_f64p(self.covars_), self.n_components, self.n_features, C.byref(handle))
            if rc == _ffi.ERR_ARG:
                raise ValueError("not a valid Gaussian HMM: " + _ffi.last_error())
            _ffi.check(rc)
            self._handle = handle
            self._finalizer = weakref.finalize(self, _release_hmm, handle)
        return self._handle

    @staticmethod
    def _offsets(lengths, n):
        if lengths is None:
            return np.array([0, n], dtype=np.int64)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lengths.shape[0] < 1 or np.any(lengths < 1) or int(lengths.sum()) != n:
            raise ValueError("lengths must be positive and sum to the %d rows of X" % n)
        return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)

    def decode(self, X, lengths=None):
        """X [n_windows][n_dims] -> (log-probability of the best path, states); with lengths, the log-probabilities of
        the sequences summed, as hmmlearn's decode."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if X.shape[1] != self.n_features or X.shape[0] < 1:
            raise ValueError("X of shape %s for a model of %d dims" % (X.shape, self.n_features))
        logprob, states = self.decode_sequences(X, lengths)
        return float(logprob.sum()), states

    def decode_sequences(self, X, lengths=None):
        """(log-probability of every sequence, states) of the rows of X [n_windows][n_dims]."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        F = np.ascontiguousarray(X.T)
        n = F.shape[1]
        offsets = self._offsets(lengths, n)
        states = np.empty(n, dtype=np.int32)
        logprob = np.empty(offsets.shape[0] - 1)
        _ffi.check(_ffi.lib().paa_hmm_decode_f64(self.handle, _ffi.as_f64p(F), self.n_features, n, n, _ffi.as_i64p(offsets),
                                                 offsets.shape[0] - 1, states.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(logprob)))
        return logprob, states.astype(np.int64)

    def predict(self, X, lengths=None):
        return self.decode(X, lengths)[1]

    def predict_device(self, d_feats, ld, n_vec, offsets=None, block_rows=None):
        """The same on a device-resident feature-major matrix (a DeviceBuffer of [n_dims][ld] doubles): (log-probability of
        every sequence, states).  offsets [n_seq + 1] cuts the windows into sequences; block_rows (tests): the block
        length of the decoder instead of its own."""
        offsets = np.array([0, n_vec], dtype=np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        n_seq = offsets.shape[0] - 1
        d_states = _ffi.DeviceBuffer(max(4 * n_vec, 8))
        d_logprob = _ffi.DeviceBuffer(8 * max(n_seq, 1))
        try:
            lib = _ffi.lib()
            if block_rows is None:
                rc = lib.paa_hmm_dev_decode_f64(self.handle, d_feats.ptr, self.n_features, ld, n_vec, _ffi.as_i64p(offsets),
                                                n_seq, d_states.ptr, d_logprob.ptr)
            else:
                rc = lib.paa_debug_hmm_dev_decode_f64(self.handle, d_feats.ptr, self.n_features, ld, n_vec,
                                                      _ffi.as_i64p(offsets), n_seq, d_states.ptr, d_logprob.ptr, block_rows)
            _ffi.check(rc)
            states = d_states.to_host(np.int32, n_vec)
            logprob = d_logprob.to_host(np.float64, n_seq)
        finally:
            d_states.free()
            d_logprob.free()
        return logprob, states.astype(np.int64)

    def log_likelihood_device(self, d_feats, ld, n_vec):
        """Frame log-likelihoods [n_vec][n_states] of a device-resident feature-major matrix."""
        d_out = _ffi.DeviceBuffer(8 * n_vec * self.n_components)
        try:
            _ffi.check(_ffi.lib().paa_hmm_dev_loglik_f64(self.handle, d_feats.ptr, self.n_features, ld, n_vec, d_out.ptr))
            return d_out.to_host(np.float64, n_vec * self.n_components).reshape(n_vec, self.n_components)
        finally:
            d_out.free()


def as_gaussian_hmm(model):
    """A GaussianHmm as it is; any other object (hmmlearn's GaussianHMM, the stand-in load_hmm builds from a reference
    file) through its startprob_, transmat_, means_ and _covars_ (hmmlearn's storage of covars_) attributes."""
    if isinstance(model, GaussianHmm):
        return model
    state = getattr(model, "__dict__", {})
    covars = state["_covars_"] if "_covars_" in state else getattr(model, "covars_")
    return GaussianHmm(model.startprob_, model.transmat_, model.means_, covars)


def _stats_labels(features, labels):
    """The reference's label handling (:302-309, :319-320): K = the number of distinct labels, labels longer than the
    matrix are cut; the transition matrix is indexed by the raw labels, so anything but 0..K-1 is an IndexError."""
    labels = np.asarray(labels)
    unique_labels = np.unique(labels)
    n_comps = len(unique_labels)
    if features.shape[1] < labels.shape[0]:
        print("trainHMM warning: number of short-term feature vectors "
              "must be greater or equal to the labels length!")
        labels = labels[0:features.shape[1]]
    if labels.shape[0] < 1:
        raise ValueError("no labelled windows")
    as_int = labels.astype(np.int64)
    if np.any(as_int != labels) or not np.array_equal(unique_labels, np.arange(n_comps)):
        raise IndexError("labels must be the integers 0..%d: the transition matrix is indexed by them" % (n_comps - 1))
    return np.ascontiguousarray(as_int, dtype=np.int32), n_comps


def train_hmm_compute_statistics(features, labels):
    """(class priors [K], transition matrix [K][K], means [K][n_dims], standard deviations [K][n_dims]) of a feature
    matrix [n_dims][n_windows] and its class indices, on the GPU (reference :287-344)."""
    F = np.ascontiguousarray(np.asarray(features, dtype=np.float64))
    if F.ndim != 2:
        raise ValueError("features must be (n_dims x n_windows)")
    lab, k = _stats_labels(F, labels)
    n = lab.shape[0]
    priors, trans = np.empty(k), np.empty((k, k))
    means, cov = np.empty((k, F.shape[0])), np.empty((k, F.shape[0]))
    _ffi.check(_ffi.lib().paa_hmm_train_stats_f64(_ffi.as_f64p(F), F.shape[0], F.shape[1], n, lab.ctypes.data_as(_ffi.c_i32p),
                                                  k, _ffi.as_f64p(priors), _ffi.as_f64p(trans), _ffi.as_f64p(means),
                                                  _ffi.as_f64p(cov)))
    return priors, trans, means, cov


def train_hmm_compute_statistics_device(d_feats, n_dims, ld, n_vec, labels):
    """The same on a device-resident feature-major matrix (labels no longer than n_vec)."""
    lab, k = _stats_labels(np.empty((n_dims, n_vec)), labels)
    priors, trans = np.empty(k), np.empty((k, k))
    means, cov = np.empty((k, n_dims)), np.empty((k, n_dims))
    _ffi.check(_ffi.lib().paa_hmm_dev_train_stats_f64(d_feats.ptr, n_dims, ld, lab.shape[0], lab.ctypes.data_as(_ffi.c_i32p), k,
                                                      _ffi.as_f64p(priors), _ffi.as_f64p(trans), _ffi.as_f64p(means),
                                                      _ffi.as_f64p(cov)))
    return priors, trans, means, cov


def save_hmm(hmm_model_name, model, classes, mid_window, mid_step):
    """Four consecutive pickles, as the reference (:455-461): model, class names, mid-term window, mid-term step."""
    import pickle
    with open(hmm_model_name, "wb") as f_handle:
        for obj in (model, classes, mid_window, mid_step):
            pickle.dump(obj, f_handle, protocol=pickle.HIGHEST_PROTOCOL)


class _HmmStandIn:
    """What a pickled hmmlearn object is rebuilt as: a bare attribute holder."""

    def __setstate__(self, state):
        self.__dict__.update(state)


def _hmm_unpickler(f_handle):
    import pickle

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            if (module, name) in (("hmmlearn.hmm", "GaussianHMM"), ("hmmlearn.base", "ConvergenceMonitor")):
                return type(name, (_HmmStandIn,), {})
            if (module, name) == (__name__, "GaussianHmm"):
                return GaussianHmm
            if (module, name) == ("collections", "deque"):
                import collections
                return collections.deque
            if (module, name) in (("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                                  ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                                  ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
                                  ("numpy", "ndarray"), ("numpy", "dtype")):
                return pickle.Unpickler.find_class(self, module, name)
            raise pickle.UnpicklingError("HMM model file names %s.%s, which a model file has no use for" % (module, name))
    return Unpickler(f_handle)


def load_hmm(hmm_model_name):
    """(GaussianHmm, class names, mid-term window, mid-term step) of a file written by save_hmm here or by the reference
    (a pickled hmmlearn GaussianHMM; hmmlearn is not needed).  Any other global in the file is refused."""
    with open(hmm_model_name, "rb") as f_handle:
        unpickler = _hmm_unpickler(f_handle)
        model = unpickler.load()
        class_names = unpickler.load()
        mid_window = unpickler.load()
        mid_step = unpickler.load()
    return as_gaussian_hmm(model), class_names, mid_window, mid_step


def _train_and_save(features, flags, class_names, hmm_model_name, mid_window, mid_step):
    class_priors, transmutation_matrix, means, cov = train_hmm_compute_statistics(features, flags)
    hmm = GaussianHmm(class_priors, transmutation_matrix, means, cov)
    save_hmm(hmm_model_name, hmm, class_names, mid_window, mid_step)
    return hmm, class_names


def train_hmm_from_file(wav_file, gt_file, hmm_model_name, mid_window, mid_step):
    """Train an HMM segmenter on one annotated file and store it (reference :347-388): returns (hmm, class_names)."""
    from . import MidTermFeatures
    seg_start, seg_end, seg_labs = read_segmentation_gt(gt_file)
    flags, class_names = segments_to_labels(seg_start, seg_end, seg_labs, mid_step)
    sampling_rate, signal = audioBasicIO.read_audio_file(wav_file)
    results, _ = MidTermFeatures._mid_for_files([(sampling_rate, signal)], mid_window, mid_step, 0.050, 0.050, False)
    return _train_and_save(results[0][0], flags, class_names, hmm_model_name, mid_window, mid_step)


def train_hmm_from_directory(folder_path, hmm_model_name, mid_window, mid_step):
    """Train an HMM segmenter on every WAV of a folder that has a .segments file and store it (reference :391-452).  The
    mid-term matrices of all files come from one batched plan per sampling rate and sample layout."""
    import glob
    import os
    from . import MidTermFeatures
    flags_all = np.array([])
    class_names_all = []
    per_file, entries = [], []
    for f in glob.glob(folder_path + os.sep + '*.wav'):
        gt_file = f.replace('.wav', '.segments')
        if os.path.isfile(gt_file):
            seg_start, seg_end, seg_labs = read_segmentation_gt(gt_file)
            flags, class_names = segments_to_labels(seg_start, seg_end, seg_labs, mid_step)
            for c in class_names:
                if c not in class_names_all:
                    class_names_all.append(c)
            # the reference's re-indexing (:430-433) maps an index of class_names_all onto itself
            flags_new = [class_names_all.index(class_names_all[fl]) for fl in flags]
            per_file.append(np.array(flags_new))
            entries.append(audioBasicIO.read_audio_file(f))
    results, _ = MidTermFeatures._mid_for_files(entries, mid_window, mid_step, 0.050, 0.050, False) if entries else ([], None)
    f_all = None
    for flags, (feature_vector, _) in zip(per_file, results):
        min_sm = min(feature_vector.shape[1], len(flags))
        flags_all = np.append(flags_all, flags[0:min_sm])
        feature_vector = feature_vector[:, 0:min_sm]
        f_all = feature_vector if f_all is None else np.concatenate((f_all, feature_vector), axis=1)
    if f_all is None:
        raise UnboundLocalError("no annotated WAV file in %s" % folder_path)      # f_all is unbound in the reference (:446)
    return _train_and_save(f_all, flags_all, class_names_all, hmm_model_name, mid_window, mid_step)


def hmm_labels(signal, sampling_rate, hmm, mid_window, mid_step):
    """hmm.predict of every mid-term window of a signal (reference :472-481): the mid-term matrix stays in HBM and goes
    straight into the emission and Viterbi kernels; only the labels come back."""
    hmm = as_gaussian_hmm(hmm)
    st = round(sampling_rate * 0.050)
    mid = _mid_term_on_device(audioBasicIO.stereo_to_mono(signal), sampling_rate, mid_window, mid_step, st, st)
    hmm.handle                            # a model the library refuses fails before any feature work
    with mid as (d_mid, M):
        _, labels = hmm.predict_device(d_mid, M, M)
    return labels


def hmm_segmentation_signal(signal, sampling_rate, hmm, class_names, mid_window, mid_step, plot_results=False, gt_file=""):
    """hmm_segmentation on a signal and a loaded model: returns (labels, class_names, accuracy, cm)."""
    labels = hmm_labels(signal, sampling_rate, hmm, mid_window, mid_step)
    labels_gt, class_names_gt, accuracy, cm = load_ground_truth(gt_file, labels, class_names, mid_step, plot_results)
    return labels, class_names, accuracy, cm


def hmm_segmentation(audio_file, hmm_model_name, plot_results=False, gt_file=""):
    """Segment an audio file with a stored HMM (reference :464-492): returns (labels, class_names, accuracy, cm)."""
    sampling_rate, signal = audioBasicIO.read_audio_file(audio_file)
    hmm, class_names, mid_window, mid_step = load_hmm(hmm_model_name)
    return hmm_segmentation_signal(signal, sampling_rate, hmm, class_names, mid_window, mid_step, plot_results, gt_file)


# ---------------------------------------------------------------------------------------------------------
# speaker diarization (reference :251-284, :815-1090; the LDA branch follows in a section of its own)
# ---------------------------------------------------------------------------------------------------------
DIAR_MODELS_ENV = "PAA_DIAR_MODELS"                  # directory that holds the two speaker SVM files
DIAR_MODEL_FILES = ("svm_rbf_speaker_10", "svm_rbf_speaker_male_female")
_DIAR_MAX_K = 32
_DIAR_MAX_DIMS = 256
_LDA_ELSEWHERE = "the LDA branch (lda_dim > 0) lives in speaker_diarization_lda / speaker_diarization_lda_signal"


def evaluate_speaker_diarization(labels, labels_gt):
    """(cluster purity, speaker purity) of fix-sized cluster labels against ground-truth labels (reference :251-284): both
    sequences are cut to the shorter one; every cluster (speaker) scores the share of its windows that fall into its most
    frequent speaker (cluster), and the scores are averaged with the cluster (speaker) sizes as weights."""
    labels, labels_gt = np.asarray(labels), np.asarray(labels_gt)
    n = min(labels.shape[0], labels_gt.shape[0])
    _, mine = np.unique(labels[:n], return_inverse=True)
    _, truth = np.unique(labels_gt[:n], return_inverse=True)
    table = np.zeros((mine.max() + 1 if n else 0, truth.max() + 1 if n else 0))
    np.add.at(table, (mine, truth), 1.0)
    per_cluster, per_speaker = table.sum(axis=1), table.sum(axis=0)
    purity_cluster_m = np.sum(table.max(axis=1) / per_cluster * per_cluster) / table.sum()
    purity_speaker_m = np.sum(table.max(axis=0) / per_speaker * per_speaker) / table.sum()
    return purity_cluster_m, purity_speaker_m


def _diar_seed(d_zk, dims, n, k, rs):
    """Greedy k-means++ (2 + int(ln k) candidates per step): the k initial centres [k][dims].  All distance work runs on the
    device (paa_diar_dev_sqdist_points_f64); the draws -- rs.randint for the first centre, rs.uniform * potential looked up in
    the cumulative sum of the closest squared distances afterwards -- and the O(n) bookkeeping stay on the host."""
    lib = _ffi.lib()
    trials = 2 + int(np.log(k))
    chosen = [int(rs.randint(n))]
    first = np.array(chosen, dtype=np.int64)
    closest = np.empty((1, n))
    _ffi.check(lib.paa_diar_dev_sqdist_points_f64(d_zk.ptr, dims, n, n, _ffi.as_i64p(first), 1, _ffi.as_f64p(closest)))
    closest = closest[0]
    for _ in range(1, k):
        vals = rs.uniform(size=trials) * closest.sum()
        cand = np.ascontiguousarray(np.minimum(np.searchsorted(np.cumsum(closest), vals), n - 1), dtype=np.int64)
        d2 = np.empty((trials, n))
        _ffi.check(lib.paa_diar_dev_sqdist_points_f64(d_zk.ptr, dims, n, n, _ffi.as_i64p(cand), trials, _ffi.as_f64p(d2)))
        new = np.minimum(closest[None, :], d2)
        best = int(np.argmin(new.sum(axis=1)))
        chosen.append(int(cand[best]))
        closest = new[best]
    idx = np.array(chosen, dtype=np.int64)
    centers = np.empty((k, dims))
    _ffi.check(lib.paa_diar_dev_get_points_f64(d_zk.ptr, dims, n, n, _ffi.as_i64p(idx), k, _ffi.as_f64p(centers)))
    return centers


def _diar_silhouette(n, k, labels, a_mean, pair_sum):
    # reference :949-985 from the per-cluster pdist means and the cluster-pair distance sums
    count = np.bincount(labels, minlength=k).astype(np.float64)
    share = count / float(n)
    a, b = np.zeros(k), np.zeros(k)
    for c in range(k):
        if share[c] < 0.020:
            continue
        a[c] = a_mean[c] * share[c]
        with np.errstate(invalid="ignore", divide="ignore"):
            b[c] = min(pair_sum[c, c2] / (count[c] * count[c2]) * (share[c] + share[c2]) / 2.0 for c2 in range(k) if c2 != c)
    sil = np.array([(b[c] - a[c]) / (max(b[c], a[c]) + 1e-5) for c in range(k)])
    return a, b, sil


def _diar_check_sweep(n_dims, n, n_speakers):
    ks = list(range(2, 10)) if n_speakers <= 0 else [int(n_speakers)]
    if n < 1 or n_dims < 1 or n_dims > _DIAR_MAX_DIMS:
        raise ValueError("feature matrix of %d dims x %d windows: 1..%d dims and at least one window" % (n_dims, n, _DIAR_MAX_DIMS))
    if min(ks) < 1 or max(ks) > _DIAR_MAX_K:
        raise ValueError("%d speakers: 1..%d clusters are supported" % (ks[0], _DIAR_MAX_K))
    if n < max(ks):
        raise ValueError("%d windows are fewer than %d clusters" % (n, max(ks)))
    return ks


def _diar_sweep_device(d_zk, dims, n, ks, tol_abs, random_state, init_centers, max_iter):
    """k-means for every k of `ks` and the silhouettes (steps 5-6) on the device matrix d_zk [dims][n], as it stands: the
    per-k entries, scores and imax of the details dict."""
    lib = _ffi.lib()
    bufs = []
    try:
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        nk = len(ks)
        centers = np.zeros((nk, _DIAR_MAX_K, dims))
        for i, k in enumerate(ks):
            if init_centers is not None and k in init_centers:
                init = np.asarray(init_centers[k], dtype=np.float64)
                if init.shape != (k, dims):
                    raise ValueError("init_centers[%d] has shape %s, %s expected" % (k, init.shape, (k, dims)))
                centers[i, :k] = init
            else:
                centers[i, :k] = _diar_seed(d_zk, dims, n, k, rs)
        ks_arr = np.array(ks, dtype=np.int32)
        ks_p = ks_arr.ctypes.data_as(_ffi.c_i32p)
        d_labels = _ffi.DeviceBuffer(nk * n * 4)
        bufs.append(d_labels)
        n_iter, inertia = np.zeros(nk, dtype=np.int32), np.empty(nk)
        _ffi.check(lib.paa_diar_dev_kmeans_f64(d_zk.ptr, dims, n, n, ks_p, nk, _ffi.as_f64p(centers), tol_abs, int(max_iter),
                                               d_labels.ptr, n_iter.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(inertia)))
        labels = d_labels.to_host(np.int32, nk * n).reshape(nk, n).astype(np.int64)
        kmax = max(ks)
        a_mean = np.empty((nk, kmax))
        a_cols = np.empty((nk, kmax, dims))
        _ffi.check(lib.paa_diar_dev_dim_distances_f64(d_zk.ptr, dims, n, n, d_labels.ptr, ks_p, nk, _ffi.as_f64p(a_cols),
                                                      _ffi.as_f64p(a_mean)))
        pair = np.empty((nk, _DIAR_MAX_K, _DIAR_MAX_K))
        _ffi.check(lib.paa_diar_dev_pair_sums_f64(d_zk.ptr, dims, n, n, d_labels.ptr, ks_p, nk, _ffi.as_f64p(pair)))
        details = {"ks": ks, "labels": {}, "centers": {}, "n_iter": {}, "inertia": {}, "sil_a": {}, "sil_b": {}, "sil": {},
                   "pair_sums": {}}
        scores = []
        for i, k in enumerate(ks):
            a, b, sil = _diar_silhouette(n, k, labels[i], a_mean[i], pair[i])
            details["labels"][k] = labels[i]
            details["centers"][k] = centers[i, :k].copy()
            details["n_iter"][k] = int(n_iter[i])
            details["inertia"][k] = float(inertia[i])
            details["sil_a"][k], details["sil_b"][k], details["sil"][k] = a, b, sil
            details["pair_sums"][k] = pair[i, :k, :k].copy()
            scores.append(np.mean(sil))
        details["scores"] = np.array(scores)
        details["imax"] = int(np.argmax(scores))
        return details
    finally:
        for b in bufs:
            b.free()


def diarize_clusters_device(d_m, n_dims, n, n_speakers, *, random_state=None, init_centers=None, max_iter=300, tol=1e-4):
    """Steps 3-6 of diarize_features on a device-resident matrix (DeviceBuffer of [n_dims][n] doubles).  Returns (details, d_z):
    the details dict of diarize_features without the HMM entries, and the DeviceBuffer of the standardised, UNFILTERED
    matrix [n_dims][n] (the caller frees it)."""
    lib = _ffi.lib()
    ks = _diar_check_sweep(n_dims, n, n_speakers)
    bufs = []
    d_z = _ffi.DeviceBuffer(n_dims * n * 8)
    try:
        stats = np.empty((3, n_dims))
        _ffi.check(lib.paa_diar_dev_standardize_f64(d_m.ptr, n_dims, n, n, d_z.ptr, _ffi.as_f64p(stats)))
        colsum, pmean = np.empty(n_dims), np.empty(1)
        _ffi.check(lib.paa_diar_dev_dim_distances_f64(d_z.ptr, n_dims, n, n, None, None, 0, _ffi.as_f64p(colsum), _ffi.as_f64p(pmean)))
        kept = np.nonzero(colsum < 1.1 * np.mean(colsum))[0]
        if kept.shape[0] < 1:
            raise ValueError("no feature dimension passes the reference's distance filter (a single dimension never does)")
        dims = int(kept.shape[0])
        rows = np.ascontiguousarray(kept, dtype=np.int32)
        d_zk = _ffi.DeviceBuffer(dims * n * 8)
        bufs.append(d_zk)
        _ffi.check(lib.paa_diar_dev_select_rows_f64(d_z.ptr, n_dims, n, n, rows.ctypes.data_as(_ffi.c_i32p), dims, d_zk.ptr))
        # tol of scikit-learn: 1e-4 * mean(var(Zk, axis=0)); a standardised row has variance var / scale^2
        tol_abs = tol * float(np.mean(stats[1, kept] / stats[2, kept] ** 2))
        details = {"kept_dims": kept, "dim_colsum": colsum, "mean": stats[0], "var": stats[1], "scale": stats[2]}
        details.update(_diar_sweep_device(d_zk, dims, n, ks, tol_abs, random_state, init_centers, max_iter))
    except BaseException:
        d_z.free()
        raise
    finally:
        for b in bufs:
            b.free()
    return details, d_z


def cluster_prepared_device(d_y, n_dims, n, n_speakers, *, random_state=None, init_centers=None, max_iter=300, tol=1e-4):
    """Steps 5-6 on an already prepared device matrix (DeviceBuffer of [n_dims][n] doubles, e.g. the LDA projection): the
    k-means sweep and the silhouettes on the matrix as it stands -- no standardisation, no dimension filter.  The k-means
    tolerance is scikit-learn's tol * mean(var(Y, axis = 0)).  Returns the per-k details of diarize_clusters_device (ks, labels,
    centers, n_iter, inertia, sil_a, sil_b, sil, pair_sums, scores, imax) and "var"."""
    ks = _diar_check_sweep(n_dims, n, n_speakers)
    d_tmp = _ffi.DeviceBuffer(n_dims * n * 8)               # the standardised copy is not wanted, its statistics are
    try:
        stats = np.empty((3, n_dims))
        _ffi.check(_ffi.lib().paa_diar_dev_standardize_f64(d_y.ptr, n_dims, n, n, d_tmp.ptr, _ffi.as_f64p(stats)))
    finally:
        d_tmp.free()
    details = _diar_sweep_device(d_y, n_dims, n, ks, tol * float(np.mean(stats[1])), random_state, init_centers, max_iter)
    details["var"] = stats[1]
    return details


def median_filter5(labels):
    """scipy.signal.medfilt(labels, 5) as float64: the 5-tap median with zero-padded edges (reference :1012)."""
    x = np.asarray(labels, dtype=np.float64)
    padded = np.concatenate((np.zeros(2), x, np.zeros(2)))
    return np.median(np.stack([padded[i:i + x.shape[0]] for i in range(5)]), axis=0)


def _diarize_device(d_m, n_dims, n, n_speakers, random_state, init_centers, return_details):
    details, d_z = diarize_clusters_device(d_m, n_dims, n, n_speakers, random_state=random_state, init_centers=init_centers)
    try:
        last = details["labels"][details["ks"][-1]]
        # the reference trains the HMM on the labels its loop variable holds when the sweep ends: the LAST k, not imax
        priors, trans, means, cov = train_hmm_compute_statistics_device(d_z, n_dims, n, n, last)
        _, states = GaussianHmm(priors, trans, means, cov).predict_device(d_z, n, n)
    finally:
        d_z.free()
    cls = median_filter5(states)
    if return_details:
        details["hmm_states"] = states
        return cls, details
    return cls


def diarize_features(M, n_speakers, *, random_state=None, init_centers=None, return_details=False):
    """Steps 3-8 of the reference's speaker_diarization (:860-1012, lda_dim = 0) on a (n_dims x n_windows) matrix of mid-term
    features and SVM probabilities, on the host or in a DeviceBuffer given as (buffer, n_dims, n_windows):

      standardise over the windows (StandardScaler); keep the feature DIMENSIONS whose summed distance to the other
      dimensions is below 1.1 times the mean (the reference's "outlier removal" acts on dimensions, windows are never
      removed); k-means for k = 2..9 (or n_speakers when > 0), one initialisation each, from init_centers[k] ([k][kept
      dims]) or greedy k-means++ seeded from numpy.random.RandomState(random_state); the reference's silhouette per k
      and imax = its first maximum; then HMM smoothing (training statistics of the UNFILTERED standardised matrix and
      Viterbi) and a 5-tap median filter (zero-padded).

    As in the reference the HMM is trained on the labels of the LAST k tried (k = 9 when n_speakers <= 0), not on those of
    imax; imax only tells how many speakers the silhouette prefers.  A k whose k-means left a cluster without windows
    raises IndexError there, as train_hmm_compute_statistics does; a feature row that is constant over a cluster gives a
    zero deviation, which the HMM refuses (ValueError).  Returns the filtered labels (float64) and, with return_details,
    a dict: kept_dims, ks, per k labels / centers / n_iter / inertia / sil_a / sil_b / sil / pair_sums, scores, imax,
    hmm_states (before the median filter)."""
    if isinstance(M, tuple):
        d_m, n_dims, n = M
        return _diarize_device(d_m, int(n_dims), int(n), n_speakers, random_state, init_centers, return_details)
    F = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    if F.ndim != 2 or F.shape[1] < 1:
        raise ValueError("M must be a (n_dims x n_windows) matrix with at least one window")
    d_m = _ffi.DeviceBuffer.from_host(F)
    try:
        return _diarize_device(d_m, F.shape[0], F.shape[1], n_speakers, random_state, init_centers, return_details)
    finally:
        d_m.free()


def _diar_models(models, models_dir=None):
    """The 10-speaker and the male / female SVM as load_model 9-tuples: given, or read from two paths, or from the files
    DIAR_MODEL_FILES of `models_dir` / the directory the environment variable PAA_DIAR_MODELS names."""
    import os
    from . import audioTrainTest
    if models is None:
        folder = models_dir or os.environ.get(DIAR_MODELS_ENV)
        if not folder:
            raise FileNotFoundError("speaker_diarization needs the SVM models %s and %s: pass models=, models_dir= or set %s to "
                                    "the directory that holds them (the package ships no model files)"
                                    % (DIAR_MODEL_FILES + (DIAR_MODELS_ENV,)))
        models = tuple(os.path.join(folder, name) for name in DIAR_MODEL_FILES)
    if len(models) != 2:
        raise ValueError("models must be the pair (10-speaker SVM, male / female SVM)")
    out = []
    for m in models:
        if isinstance(m, (str, bytes, os.PathLike)):
            for path in (m, str(m) + "MEANS"):
                if not os.path.isfile(path):
                    raise FileNotFoundError("speaker diarization model file %s is missing" % path)
            m = audioTrainTest.load_model(m)
        out.append(m)
    return out


def speaker_diarization_signal(signal, sampling_rate, n_speakers, mid_window=1.0, mid_step=0.1, short_window=0.1, lda_dim=0, *,
                               models=None, models_dir=None, random_state=None, init_centers=None, return_details=False):
    """Steps 1-8 of speaker_diarization on an array: mid-term features (short window and step round(fs * 0.05); short_window
    only matters to the LDA branch), the probabilities of the two speaker SVMs + 1e-4 below them, then diarize_features -- the
    matrix never leaves the device.  models: see speaker_diarization."""
    from . import audioTrainTest
    if lda_dim > 0:
        raise NotImplementedError(_LDA_ELSEWHERE)
    loaded = _diar_models(models, models_dir)
    svcs = [(audioTrainTest.svc_model(m[0]), np.asarray(m[1], dtype=np.float64), np.asarray(m[2], dtype=np.float64)) for m in loaded]
    st = round(sampling_rate * 0.05)
    rows, extra = 2 * 68, sum(len(s[0].classes) for s in svcs)
    with _mid_term_on_device(audioBasicIO.stereo_to_mono(signal), sampling_rate, mid_window, mid_step, st, st, extra) as (d_all, M):
        at = rows                                   # the probability rows go below the mid-term rows
        for model, mean, std in svcs:
            _, proba = model.predict_device(d_all, M, M, mean, std)
            block = np.ascontiguousarray(proba.T + 1e-4)
            _ffi.check(_ffi.lib().paa_memcpy_h2d(C.c_void_p(d_all.ptr.value + at * M * 8), block.ctypes.data_as(C.c_void_p),
                                                 block.nbytes))
            at += block.shape[0]
        return _diarize_device(d_all, rows + extra, M, n_speakers, random_state, init_centers, return_details)


def _plot_diarization(cls, n_classes, duration, mid_step, flags_gt, purities, n_speakers, scores):
    import matplotlib.pyplot as plt
    names = ["speaker{0:d}".format(c) for c in range(n_classes)]
    fig = plt.figure()
    ax1 = fig.add_subplot(111 if n_speakers > 0 else 211)
    ax1.set_yticks(np.arange(len(names)))
    ax1.axis((0, duration, -1, len(names)))
    ax1.set_yticklabels(names)
    ax1.plot(np.arange(len(cls)) * mid_step + mid_step / 2.0, cls)
    if flags_gt is not None:
        ax1.plot(np.arange(len(flags_gt)) * mid_step + mid_step / 2.0, flags_gt, 'r')
        plt.title("Cluster purity: {0:.1f}% - Speaker purity: {1:.1f}%".format(100 * purities[0], 100 * purities[1]))
    plt.xlabel("time (seconds)")
    if n_speakers <= 0:
        plt.subplot(212)
        plt.plot(list(range(2, 10)), scores)
        plt.xlabel("number of clusters")
        plt.ylabel("average clustering's sillouette")
    plt.show()


def speaker_diarization(filename, n_speakers, mid_window=1.0, mid_step=0.1, short_window=0.1, lda_dim=0, plot_res=False, *,
                        models=None, models_dir=None, random_state=None, init_centers=None):
    """Speaker diarization of a WAV file (reference :815-1056, lda_dim = 0; lda_dim > 0: speaker_diarization_lda): returns
    (cls, purity_cluster_m, purity_speaker_m) -- the label of every mid-term window (float64) and, when <filename>.segments exists next to the file,
    the cluster and speaker purity against it (printed as the reference prints them), else -1, -1.

    n_speakers <= 0 sweeps k = 2..9.  As in the reference the returned labels come from the k-means of the LAST k tried,
    smoothed by an HMM and a median filter (see diarize_features); the silhouette's choice only sets the number of class
    names of the plot.  models: the pair (10-speaker SVM, male / female SVM) as load_model 9-tuples or as two paths; None
    reads svm_rbf_speaker_10 and svm_rbf_speaker_male_female (and their MEANS files) from models_dir or the directory
    named by the environment variable PAA_DIAR_MODELS -- FileNotFoundError says what is missing.  random_state seeds the
    k-means++ initialisation (the reference leaves it unseeded); init_centers {k: [k][kept dims]} replaces it."""
    if lda_dim > 0:
        raise NotImplementedError(_LDA_ELSEWHERE)
    loaded = _diar_models(models, models_dir)
    sampling_rate, signal = audioBasicIO.read_audio_file(filename)
    signal = audioBasicIO.stereo_to_mono(signal)
    duration = len(signal) / sampling_rate
    cls, details = speaker_diarization_signal(signal, sampling_rate, n_speakers, mid_window, mid_step, short_window, lda_dim,
                                              models=loaded, random_state=random_state, init_centers=init_centers,
                                              return_details=True)
    return _score_diarization(filename, cls, details, mid_step, duration, n_speakers, plot_res)


def _score_diarization(filename, cls, details, mid_step, duration, n_speakers, plot_res):
    """(cls, cluster purity, speaker purity) against <filename>.segments when it exists (printed as the reference prints
    them), else -1, -1; the plot on request (reference :1014-1056)."""
    import os
    purities = (-1, -1)
    flags_gt = None
    gt_file = filename.replace('.wav', '.segments')
    if os.path.isfile(gt_file):
        seg_start, seg_end, seg_labs = read_segmentation_gt(gt_file)
        flags_gt, _ = segments_to_labels(seg_start, seg_end, seg_labs, mid_step)
        purities = evaluate_speaker_diarization(cls, flags_gt)
        print("{0:.1f}\t{1:.1f}".format(100 * purities[0], 100 * purities[1]))
    if plot_res:
        _plot_diarization(cls, details["ks"][details["imax"]], duration, mid_step, flags_gt, purities, n_speakers,
                          details["scores"])
    return cls, purities[0], purities[1]


def speaker_diarization_evaluation(folder_name, lda_dimensions, *, models=None, models_dir=None, random_state=None, batch=False):
    """Prints the purities of every WAV file of a folder for every LDA dimension of the list (reference :1059-1090): the
    number of speakers comes from the file's .segments ground truth (-1: unknown).  Dimension 0 runs speaker_diarization,
    a dimension above 0 speaker_diarization_lda, both with the reference's settings (2.0 / 0.2 / 0.05 s).  batch=True sends
    the dimension-0 pass through speaker_diarization_files: one device batch per sampling rate, the same lines printed."""
    import glob
    import os
    wav_files = sorted(glob.glob(os.path.join(folder_name, '*.wav')))
    loaded = _diar_models(models, models_dir)
    num_speakers = []
    for wav_file in wav_files:
        gt_file = wav_file.replace('.wav', '.segments')
        if os.path.isfile(gt_file):
            _, _, seg_labs = read_segmentation_gt(gt_file)
            num_speakers.append(len(set(seg_labs)))
        else:
            num_speakers.append(-1)
    for dim in lda_dimensions:
        print("LDA = {0:d}".format(dim))
        if batch and dim <= 0:
            speaker_diarization_files(wav_files, num_speakers, 2.0, 0.2, 0.05, dim, plot_res=False, models=loaded,
                                      random_state=random_state)
            continue
        for i, wav_file in enumerate(wav_files):
            if dim > 0:
                speaker_diarization_lda(wav_file, num_speakers[i], 2.0, 0.2, 0.05, dim, plot_res=False, models=loaded,
                                        random_state=random_state)
            else:
                speaker_diarization(wav_file, num_speakers[i], 2.0, 0.2, 0.05, dim, plot_res=False, models=loaded,
                                    random_state=random_state)


# ---------------------------------------------------------------------------------------------------------
# speaker diarization of many clips in one call (lda_dim = 0)
# ---------------------------------------------------------------------------------------------------------
_DIAR_BATCH_MAX_JOBS = 8192        # (clip, k) jobs and (job, cluster) slots of one chunk: every grid stays below the y limit
_DIAR_BATCH_MAX_SLOTS = 65535
_DIAR_PAIR_TILE = 128              # kernels_diarbatch.hpp: windows per side of a pair tile, tiles per first-stage sum
_DIAR_PAIR_CHUNK = 256


class _DeviceView:
    """Columns of a device matrix as the object the single-clip entry points take: .ptr, nothing owned."""

    def __init__(self, buf, offset_bytes):
        self.ptr = C.c_void_p(buf.ptr.value + int(offset_bytes))


def _diar_batch_ks(n_speakers):
    return list(range(2, 10)) if n_speakers <= 0 else [int(n_speakers)]


def _diar_batch_check(n_dims_list, ns, n_speakers, init_centers):
    """The argument half of diarize_features_batch, without the device: (n_dims, ks per clip, init_centers per clip) or the
    ValueError of the first clip that cannot be served, named by its index."""
    n_clips = len(ns)
    if np.ndim(n_speakers) == 0:
        speakers = [int(n_speakers)] * n_clips
    else:
        speakers = [int(s) for s in n_speakers]
        if len(speakers) != n_clips:
            raise ValueError("n_speakers: an int or one int per clip (%d clips, %d values)" % (n_clips, len(speakers)))
    if init_centers is None:
        inits = [None] * n_clips
    else:
        inits = list(init_centers)
        if len(inits) != n_clips:
            raise ValueError("init_centers: None or one dict (or None) per clip (%d clips, %d entries)" % (n_clips, len(inits)))
    n_dims = int(n_dims_list[0]) if n_clips else 0
    ks_list = []
    for c in range(n_clips):
        d, n = int(n_dims_list[c]), int(ns[c])
        if d != n_dims:
            raise ValueError("clip %d: %d feature dims, clip 0 has %d (one batch shares n_dims)" % (c, d, n_dims))
        if d < 1 or d > _DIAR_MAX_DIMS or n < 1:
            raise ValueError("clip %d: feature matrix of %d dims x %d windows: 1..%d dims and at least one window"
                             % (c, d, n, _DIAR_MAX_DIMS))
        ks = _diar_batch_ks(speakers[c])
        if min(ks) < 1 or max(ks) > _DIAR_MAX_K:
            raise ValueError("clip %d: %d speakers: 1..%d clusters are supported" % (c, ks[0], _DIAR_MAX_K))
        if n < max(ks):
            raise ValueError("clip %d: %d windows are fewer than %d clusters" % (c, n, max(ks)))
        if inits[c] is not None:
            checked = {}
            for k, init in dict(inits[c]).items():
                init = np.asarray(init, dtype=np.float64)
                if k in ks and (init.ndim != 2 or init.shape[0] != k or not 1 <= init.shape[1] <= d):
                    raise ValueError("clip %d: init_centers[%d] has shape %s, (%d, kept dims <= %d) expected" % (c, k, init.shape, k, d))
                checked[k] = init
            inits[c] = checked
        ks_list.append(ks)
    return n_dims, ks_list, inits


def _diar_clip_bytes(n_dims, n, ks):
    """Device scratch of one clip's jobs in paa_diar_batch_sweep_f64 (labels, d2, the seeding's candidate rows, the feature-row
    distance matrices with every row kept, the pair partials and their first-stage sums) and in paa_diar_batch_prepare_f64."""
    nb = (n + _DIAR_PAIR_TILE - 1) // _DIAR_PAIR_TILE
    tiles = nb * (nb + 1) // 2
    bins = sum(k * k for k in ks)
    trials = sum(2 + int(np.log(k)) for k in ks)
    return (12 * len(ks) + 8 * trials) * n + 8 * (tiles + (tiles + _DIAR_PAIR_CHUNK - 1) // _DIAR_PAIR_CHUNK + 1) * bins \
        + 8 * (sum(ks) + 1) * n_dims * n_dims + 8 * 2 * sum(ks) * n_dims


def _diar_batch_chunks(n_dims, ns, ks_list, chunk_bytes=None):
    """Clips packed into chunks in order: [(first, last + 1)].  A chunk's scratch stays under chunk_bytes (1 GiB when None) and
    its jobs under _DIAR_BATCH_MAX_JOBS; a clip that is over the bound by itself is a chunk of one."""
    bound = int(chunk_bytes) if chunk_bytes else 1 << 30
    chunks, first, used, jobs, slots = [], 0, 0, 0, 0
    for c in range(len(ns)):
        need = _diar_clip_bytes(n_dims, int(ns[c]), ks_list[c])
        if c > first and (used + need > bound or jobs + len(ks_list[c]) > _DIAR_BATCH_MAX_JOBS
                          or slots + sum(ks_list[c]) > _DIAR_BATCH_MAX_SLOTS):
            chunks.append((first, c))
            first, used, jobs, slots = c, 0, 0, 0
        used += need
        jobs += len(ks_list[c])
        slots += sum(ks_list[c])
    if len(ns) > first:
        chunks.append((first, len(ns)))
    return chunks


def _diar_batch_draws(rs, n, ks, init, dims=None):
    """What one clip's sweep takes from `rs`, drawn up front in the order of the loop: per k without given centres randint(n),
    then (k - 1) times uniform(size = 2 + int(ln k)) -- the count does not depend on the data.  Returns ([(k, first, u)], exc):
    a given init_centers[k] whose shape is not (k, dims) stops the draws where the loop would raise, and exc is that ValueError
    (dims None: the shapes are not looked at)."""
    out = []
    for k in ks:
        if init is not None and k in init:
            if dims is not None and init[k].shape != (k, dims):
                return out, ValueError("init_centers[%d] has shape %s, %s expected" % (k, init[k].shape, (k, dims)))
            out.append((k, None, None))
            continue
        trials = 2 + int(np.log(k))
        first = int(rs.randint(n))
        u = np.empty((k - 1, trials))
        for step in range(k - 1):
            u[step] = rs.uniform(size=trials)
        out.append((k, first, u))
    return out, None


def _diar_sweep_chunk(d_z, n_dims, ld, cols, ns, kept_list, tols, draws_list, inits, max_iter, d_labels, stage_ms):
    """paa_diar_batch_sweep_f64 for the clips of one chunk (all of them good): per clip the per-k half of the details dict"""
    lib = _ffi.lib()
    n_clips = len(ns)
    dims = np.array([len(k) for k in kept_list], dtype=np.int32)
    rows = np.ascontiguousarray(np.concatenate(kept_list), dtype=np.int32)
    nks = np.array([len(d) for d in draws_list], dtype=np.int32)
    ks = np.array([k for d in draws_list for k, _, _ in d], dtype=np.int32)
    n_jobs = ks.shape[0]
    seeded, first = np.zeros(n_jobs, dtype=np.int32), np.zeros(n_jobs, dtype=np.int64)
    us, cen, cen_off, job = [], [], [0], 0
    for c, draws in enumerate(draws_list):
        for k, f, u in draws:
            if f is None:
                cen.append(np.ascontiguousarray(inits[c][k], dtype=np.float64).reshape(-1))
            else:
                seeded[job], first[job] = 1, f
                us.append(u.reshape(-1))
                cen.append(np.zeros(k * int(dims[c])))
            cen_off.append(cen_off[-1] + k * int(dims[c]))
            job += 1
    centers = np.ascontiguousarray(np.concatenate(cen))
    u_all = np.ascontiguousarray(np.concatenate(us)) if us else np.zeros(1)
    n_iter, inertia = np.zeros(n_jobs, dtype=np.int32), np.empty(n_jobs)
    a_mean, pair = np.empty((n_jobs, _DIAR_MAX_K)), np.empty((n_jobs, _DIAR_MAX_K, _DIAR_MAX_K))
    ms = np.zeros(4)
    _ffi.check(lib.paa_diar_batch_sweep_f64(
        d_z.ptr, n_dims, ld, n_clips, _ffi.as_i64p(np.ascontiguousarray(cols, dtype=np.int64)),
        _ffi.as_i64p(np.ascontiguousarray(ns, dtype=np.int64)), _ffi.as_i32p(dims), _ffi.as_i32p(rows), _ffi.as_i32p(nks), _ffi.as_i32p(ks),
        _ffi.as_f64p(np.ascontiguousarray(tols, dtype=np.float64)), int(max_iter), _ffi.as_i32p(seeded), _ffi.as_i64p(first),
        _ffi.as_f64p(u_all), _ffi.as_f64p(centers), d_labels.ptr, _ffi.as_i32p(n_iter), _ffi.as_f64p(inertia), _ffi.as_f64p(a_mean),
        _ffi.as_f64p(pair), _ffi.as_f64p(ms) if stage_ms is not None else None))
    if stage_ms is not None:
        for name, v in zip(("seeding", "kmeans", "silhouette_inputs"), ms[:3]):
            stage_ms[name] = stage_ms.get(name, 0.0) + float(v)
        stage_ms["kmeans_rounds"] = stage_ms.get("kmeans_rounds", 0) + int(ms[3])
    total = int(sum(int(nks[c]) * int(ns[c]) for c in range(n_clips)))
    t0 = time.perf_counter()
    labels_all = d_labels.to_host(np.int32, total)                 # ONE read-back for the labels of every job of the chunk
    if stage_ms is not None:
        stage_ms["copy_back"] = stage_ms.get("copy_back", 0.0) + 1e3 * (time.perf_counter() - t0)
    out, job, at = [], 0, 0
    for c, draws in enumerate(draws_list):
        n = int(ns[c])
        details = {"ks": [k for k, _, _ in draws], "labels": {}, "centers": {}, "n_iter": {}, "inertia": {}, "sil_a": {}, "sil_b": {},
                   "sil": {}, "pair_sums": {}}
        scores = []
        for k, _, _ in draws:
            labels = labels_all[at:at + n].astype(np.int64)
            a, b, sil = _diar_silhouette(n, k, labels, a_mean[job], pair[job])
            details["labels"][k] = labels
            details["centers"][k] = centers[cen_off[job]:cen_off[job + 1]].reshape(k, int(dims[c])).copy()
            details["n_iter"][k] = int(n_iter[job])
            details["inertia"][k] = float(inertia[job])
            details["sil_a"][k], details["sil_b"][k], details["sil"][k] = a, b, sil
            details["pair_sums"][k] = pair[job, :k, :k].copy()
            scores.append(np.mean(sil))
            job += 1
            at += n
        details["scores"] = np.array(scores)
        details["imax"] = int(np.argmax(scores))
        out.append(details)
    return out


def diarize_clusters_batch_device(d_m, n_dims, ld, cols, ns, n_speakers, *, random_state=None, init_centers=None, max_iter=300,
                                  tol=1e-4, chunk_bytes=None):
    """The batch form of diarize_clusters_device: steps 3-6 of diarize_features for MANY clips that lie side by side in one
    device matrix (DeviceBuffer of [n_dims][ld] doubles, clip c in the columns cols[c] .. cols[c] + ns[c] - 1).  Returns
    (results, d_z): per clip the details dict of diarize_clusters_device -- or the exception its single call would raise (no
    dimension passes the filter, an init_centers entry of the wrong shape) -- and the DeviceBuffer of the standardised,
    UNFILTERED matrix [n_dims][ld] (the caller frees it).  Clip c's entries equal its own single call bit for bit.

    Per chunk of clips (chunk_bytes bounds the device scratch, 1 GiB when None) the host waits once for the standardisation
    and the dimension distances of all clips, once per Lloyd iteration of the slowest (clip, k) job, and twice for the
    silhouette inputs and the labels.  The filter colsum < 1.1 * mean, the k-means tolerance and the silhouette arithmetic stay
    in NumPy on the host, so their bits are the loop's.  The k-means++ draws are made up front in clip order (see
    _diar_batch_draws): an int random_state seeds every clip afresh, a RandomState instance is consumed as the loop would."""
    return _diar_clusters_batch(d_m, n_dims, ld, cols, ns, n_speakers, random_state, init_centers, max_iter, tol, chunk_bytes)


def _diar_clusters_batch(d_m, n_dims, ld, cols, ns, n_speakers, random_state, init_centers, max_iter=300, tol=1e-4, chunk_bytes=None,
                         stage_ms=None, given_draws=None):
    """diarize_clusters_batch_device; stage_ms: a dict that collects the milliseconds per stage (the benchmark's), given_draws:
    per clip the draws its caller made in ITS clip order (speaker_diarization_files)"""
    lib = _ffi.lib()
    cols, ns = np.ascontiguousarray(cols, dtype=np.int64), np.ascontiguousarray(ns, dtype=np.int64)
    n_clips = ns.shape[0]
    _, ks_list, inits = _diar_batch_check([n_dims] * n_clips, ns, n_speakers, init_centers)
    results = [None] * n_clips
    d_z = _ffi.DeviceBuffer(n_dims * ld * 8)
    d_labels = None
    try:
        for lo, hi in _diar_batch_chunks(n_dims, ns, ks_list, chunk_bytes):
            m = hi - lo
            stats, colsum = np.empty((m, 3, n_dims)), np.empty((m, n_dims))
            t0 = time.perf_counter()
            _ffi.check(lib.paa_diar_batch_prepare_f64(d_m.ptr, n_dims, ld, _ffi.as_i64p(cols[lo:hi].copy()), _ffi.as_i64p(ns[lo:hi].copy()),
                                                      m, d_z.ptr, _ffi.as_f64p(stats), _ffi.as_f64p(colsum)))
            if stage_ms is not None:
                stage_ms["prepare"] = stage_ms.get("prepare", 0.0) + 1e3 * (time.perf_counter() - t0)
            good, kept_list, tols, draws_list, heads = [], [], [], [], {}
            for c in range(lo, hi):
                cs, st = colsum[c - lo], stats[c - lo]
                kept = np.nonzero(cs < 1.1 * np.mean(cs))[0]
                if kept.shape[0] < 1:
                    results[c] = ValueError("no feature dimension passes the reference's distance filter (a single dimension never does)")
                    continue
                if given_draws is not None:
                    exc = None
                    for k, f, u in given_draws[c]:
                        if f is None and inits[c][k].shape != (k, int(kept.shape[0])):
                            exc = ValueError("init_centers[%d] has shape %s, %s expected" % (k, inits[c][k].shape, (k, int(kept.shape[0]))))
                            break
                    draws = given_draws[c]
                else:
                    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
                    draws, exc = _diar_batch_draws(rs, int(ns[c]), ks_list[c], inits[c], int(kept.shape[0]))
                if exc is not None:
                    results[c] = exc
                    continue
                good.append(c)
                kept_list.append(kept)
                # tol of scikit-learn: 1e-4 * mean(var(Zk, axis=0)); a standardised row has variance var / scale^2
                tols.append(tol * float(np.mean(st[1, kept] / st[2, kept] ** 2)))
                draws_list.append(draws)
                heads[c] = {"kept_dims": kept, "dim_colsum": cs.copy(), "mean": st[0].copy(), "var": st[1].copy(), "scale": st[2].copy()}
            if not good:
                continue
            total = int(sum(len(ks_list[c]) * int(ns[c]) for c in good))
            d_labels = _ffi.DeviceBuffer(max(4 * total, 8))
            swept = _diar_sweep_chunk(d_z, n_dims, ld, cols[good], ns[good], kept_list, tols, draws_list, [inits[c] for c in good], max_iter,
                                      d_labels, stage_ms)
            d_labels.free()
            d_labels = None
            for c, details in zip(good, swept):
                heads[c].update(details)
                results[c] = heads[c]
    except BaseException:
        d_z.free()
        raise
    finally:
        if d_labels is not None:
            d_labels.free()
    return results, d_z


def diarize_hmm_batch_device(d_z, n_dims, ld, cols, ns, labels_list):
    """The HMM smoothing of a batch alone (steps 7-8 before the median filter): per clip the Viterbi states of the HMM trained
    on that clip's columns of the device matrix d_z [n_dims][ld] and its labels -- or the exception the single call raises
    (IndexError: a cluster without windows; ValueError: a zero deviation or a state that is never left).  labels_list[c] is
    None for a clip to skip (its slot stays None).  The clips run one after the other through the single-clip entry points
    (train_hmm_compute_statistics_device, GaussianHmm.predict_device) on the resident matrix: this stage still waits per clip."""
    out = [None] * len(ns)
    for c, labels in enumerate(labels_list):
        if labels is None:
            continue
        view = _DeviceView(d_z, 8 * int(cols[c]))
        try:
            priors, trans, means, cov = train_hmm_compute_statistics_device(view, n_dims, ld, int(ns[c]), labels)
            _, out[c] = GaussianHmm(priors, trans, means, cov).predict_device(view, ld, int(ns[c]))
        except (ValueError, IndexError) as exc:
            out[c] = exc
    return out


def _diar_batch_finish(results, states, return_details, on_error):
    """per clip (cls, details) or the exception; on_error = "raise" raises the first exception, named by its clip"""
    out = []
    for c, (details, st) in enumerate(zip(results, states)):
        failed = details if isinstance(details, BaseException) else st if isinstance(st, BaseException) else None
        if failed is not None:
            failed.details = None if failed is details else details      # what the clustering gave before the HMM refused
            if on_error == "raise":
                raise type(failed)("clip %d: %s" % (c, failed))
            out.append(failed)
            continue
        cls = median_filter5(st)
        if return_details:
            details["hmm_states"] = st
            out.append((cls, details))
        else:
            out.append(cls)
    return out


def _diarize_batch_device(d_m, n_dims, ld, cols, ns, n_speakers, random_state, init_centers, return_details, on_error, chunk_bytes,
                          stage_ms=None, draws=None):
    if on_error not in ("raise", "record"):
        raise ValueError("on_error must be 'raise' or 'record', not %r" % (on_error,))
    results, d_z = _diar_clusters_batch(d_m, n_dims, ld, cols, ns, n_speakers, random_state, init_centers, chunk_bytes=chunk_bytes,
                                        stage_ms=stage_ms, given_draws=draws)
    try:
        t0 = time.perf_counter()
        # the reference trains the HMM on the labels its loop variable holds when the sweep ends: the LAST k, not imax
        last = [None if isinstance(r, BaseException) else r["labels"][r["ks"][-1]] for r in results]
        states = diarize_hmm_batch_device(d_z, n_dims, ld, cols, ns, last)
        if stage_ms is not None:
            stage_ms["hmm"] = stage_ms.get("hmm", 0.0) + 1e3 * (time.perf_counter() - t0)
    finally:
        d_z.free()
    return _diar_batch_finish(results, states, return_details, on_error)


def diarize_features_batch(mats, n_speakers, *, random_state=None, init_centers=None, return_details=False, on_error="raise",
                           chunk_bytes=None):
    """diarize_features for a list of (n_dims x n_c) matrices with the same n_dims and ragged n_c, as ONE device batch: the
    matrices lie side by side in one device matrix, and standardisation, the dimension distances, k-means++ seeding, k-means
    over all (clip, k) jobs, the per-cluster dimension distances and the cluster-pair sums are each one launch (k-means: one
    per Lloyd iteration) over every clip of a chunk -- see diarize_clusters_batch_device for what the host waits for.  The
    HMM smoothing runs clip by clip on the resident matrix (diarize_hmm_batch_device).

    n_speakers: an int or one int per clip, <= 0 sweeps k = 2..9 for that clip.  init_centers: None, or one {k: [k][kept
    dims]} dict (or None) per clip.  random_state: an int seeds every clip afresh, as a loop of diarize_features calls with
    that int; a numpy.random.RandomState is consumed in clip order exactly as that loop would consume it.  Returns a list: per
    clip what diarize_features returns (with return_details the (labels, details) pair), EQUAL to that clip's own call bit for
    bit at any position, beside any other clips and under any chunk_bytes (a bound on the device scratch of one chunk of clips,
    1 GiB when None).

    ValueError names the clip and comes before any device work: differing n_dims, n_dims outside 1..256, k outside 1..32, fewer
    windows than the largest k, an init_centers entry that cannot be [k][kept dims].  What the loop raises from the data -- no
    dimension passes the filter (ValueError), an init_centers entry whose width is not the kept dims (ValueError), a cluster
    of the last k without windows (IndexError), a zero deviation or a never-left state in the HMM (ValueError) -- is raised
    after the batch has run, named by its clip (on_error="raise", the first of them), or put into that clip's slot as the
    exception object while every other clip's result stays intact (on_error="record"; when it was the HMM that refused, the
    exception's .details holds the clustering details of that clip).  An empty list returns []."""
    mats = [np.asarray(m, dtype=np.float64) for m in mats]
    if not mats:
        return []
    for c, m in enumerate(mats):
        if m.ndim != 2 or m.shape[1] < 1:
            raise ValueError("clip %d: M must be a (n_dims x n_windows) matrix with at least one window" % c)
    if on_error not in ("raise", "record"):
        raise ValueError("on_error must be 'raise' or 'record', not %r" % (on_error,))
    ns = np.array([m.shape[1] for m in mats], dtype=np.int64)
    n_dims, _, _ = _diar_batch_check([m.shape[0] for m in mats], ns, n_speakers, init_centers)
    cols = np.concatenate(([0], np.cumsum(ns)[:-1])).astype(np.int64)
    d_m = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(np.concatenate(mats, axis=1)))
    try:
        return _diarize_batch_device(d_m, n_dims, int(ns.sum()), cols, ns, n_speakers, random_state, init_centers, return_details,
                                     on_error, chunk_bytes)
    finally:
        d_m.free()


def _diar_batch_plan(lengths, sampling_rate, mid_window, mid_step):
    """The argument half of speaker_diarization_batch, without the device: (short-term window = step in samples, mid ratio, mid
    step ratio, mid-term windows per clip) or the ValueError of the first clip that cannot be served."""
    from . import MidTermFeatures
    st = round(sampling_rate * 0.05)
    ratio, step_ratio = MidTermFeatures._ratios(mid_window * sampling_rate, mid_step * sampling_rate, st, st)
    if step_ratio < 1:
        raise ValueError("mid_step / short_step rounds to 0: the reference never terminates")
    lib = _ffi.lib()
    st = int(st)
    windows = []
    for c, n in enumerate(lengths):
        if st < 1 or n < st:
            raise ValueError("clip %d: need at least one array to concatenate (%d samples, a window of %d)" % (c, n, st))
        windows.append(int(lib.paa_num_mid_windows(int(lib.paa_num_frames(int(n), st, st)), step_ratio)))
    return st, ratio, step_ratio, np.array(windows, dtype=np.int64)


def _diar_extra_rows(loaded):
    """the probability rows the two speaker SVMs add below the mid-term rows (read from the classifiers, no device copy)"""
    return sum(len(np.asarray(m[0].classes_)) for m in loaded)


def _diar_svcs(loaded):
    from . import audioTrainTest
    return [(audioTrainTest.svc_model(m[0]), np.asarray(m[1], dtype=np.float64), np.asarray(m[2], dtype=np.float64)) for m in loaded]


def _speaker_batch(monos, sampling_rate, n_speakers, mid_window, mid_step, loaded, random_state, init_centers, return_details, on_error,
                   chunk_bytes, stage_ms=None, draws=None):
    """speaker_diarization_batch on mono clips: one batched plan per sample kind writes the mid-term slabs of its clips into
    ONE device matrix [136 + extra][total windows], one predict_device call per speaker SVM covers every window of every clip,
    and the clustering batch runs on that matrix."""
    lib = _ffi.lib()
    classified = [_ffi.classify_signal(m) for m in monos]
    st, ratio, step_ratio, M = _diar_batch_plan([s.shape[0] for _, s in classified], sampling_rate, mid_window, mid_step)
    rows, extra = 2 * 68, _diar_extra_rows(loaded)
    n_dims, n = rows + extra, len(monos)
    _diar_batch_check([n_dims] * n, M, n_speakers, init_centers)
    if on_error not in ("raise", "record"):
        raise ValueError("on_error must be 'raise' or 'record', not %r" % (on_error,))
    svcs = _diar_svcs(loaded)                       # the first call that may touch the device
    cols = np.concatenate(([0], np.cumsum(M)[:-1])).astype(np.int64)
    total = int(M.sum())
    t0 = time.perf_counter()
    d_all = _ffi.DeviceBuffer(n_dims * total * 8)
    try:
        for kind in (0, 1):
            ids = [c for c in range(n) if classified[c][0] == kind]
            if not ids:
                continue
            offsets = np.zeros(len(ids) + 1, dtype=np.int64)
            np.cumsum([classified[c][1].shape[0] for c in ids], out=offsets[1:])
            plan = _ffi.Plan(offsets, sampling_rate, st, st, deltas=True, sample_kind=kind)
            bufs = []
            try:
                bufs.append(_ffi.DeviceBuffer.from_host(np.concatenate([classified[c][1] for c in ids])))
                bufs.append(_ffi.DeviceBuffer(plan.out_doubles * 8))
                plan.execute(bufs[0], bufs[1])
                n_mid = plan.mid_doubles(step_ratio)
                if n_mid != rows * int(M[ids].sum()):
                    raise RuntimeError("the batched plan has %d mid-term values, %d expected" % (n_mid, rows * int(M[ids].sum())))
                bufs.append(_ffi.DeviceBuffer(n_mid * 8))
                plan.mid_execute(bufs[1], ratio, step_ratio, bufs[2])
                slabs = np.concatenate(([0], np.cumsum(rows * M[ids])[:-1])).astype(np.int64)
                _ffi.check(lib.paa_diar_batch_gather_f64(bufs[2].ptr, rows, _ffi.as_i64p(slabs), _ffi.as_i64p(cols[ids].copy()),
                                                         _ffi.as_i64p(M[ids].copy()), len(ids), d_all.ptr, total))
            finally:
                for b in bufs:
                    b.free()
                plan.destroy()
        at = rows                                   # the probability rows go below the mid-term rows
        for model, mean, std in svcs:
            _, proba = model.predict_device(d_all, total, total, mean, std)
            block = np.ascontiguousarray(proba.T + 1e-4)
            _ffi.check(lib.paa_memcpy_h2d(C.c_void_p(d_all.ptr.value + at * total * 8), block.ctypes.data_as(C.c_void_p), block.nbytes))
            at += block.shape[0]
        if stage_ms is not None:
            stage_ms["features_svms"] = stage_ms.get("features_svms", 0.0) + 1e3 * (time.perf_counter() - t0)
        return _diarize_batch_device(d_all, n_dims, total, cols, M, n_speakers, random_state, init_centers, return_details, on_error,
                                     chunk_bytes, stage_ms, draws)
    finally:
        d_all.free()


def speaker_diarization_batch(signals, sampling_rate, n_speakers, mid_window=1.0, mid_step=0.1, short_window=0.1, lda_dim=0, *,
                              models=None, models_dir=None, random_state=None, init_centers=None, return_details=False,
                              on_error="raise", chunk_bytes=None):
    """speaker_diarization_signal for a list of clips of ONE sampling rate, on the GPU end to end: one batched plan gives the
    mid-term matrices of all clips in one [136 + extra][total windows] device matrix, ONE predict_device call per speaker SVM
    covers all windows of all clips and writes the probability rows + 1e-4 below the mid-term rows, and diarize_features_batch's
    stages run on that matrix, which never leaves the device.  Returns a list: per clip what speaker_diarization_signal returns
    for that clip alone, bit for bit.  n_speakers, random_state, init_centers, return_details, on_error and chunk_bytes: see
    diarize_features_batch; models: see speaker_diarization.  Each clip goes through audioBasicIO.stereo_to_mono; int16 clips
    travel as int16, the others through np.double.  lda_dim > 0 raises NotImplementedError, as the single call does.  An empty
    list returns [].  ValueError names the clip and comes before any device work."""
    if lda_dim > 0:
        raise NotImplementedError(_LDA_ELSEWHERE)
    signals = list(signals)
    if not signals:
        return []
    loaded = _diar_models(models, models_dir)
    return _speaker_batch(_mono_clips(signals), sampling_rate, n_speakers, mid_window, mid_step, loaded, random_state, init_centers,
                          return_details, on_error, chunk_bytes)


def speaker_diarization_files(paths, n_speakers, mid_window=1.0, mid_step=0.1, short_window=0.1, lda_dim=0, plot_res=False, *,
                              models=None, models_dir=None, random_state=None, init_centers=None, chunk_bytes=None):
    """speaker_diarization over audio files: they are read and grouped by sampling rate, one device batch per rate
    (speaker_diarization_batch), and every file is scored against its .segments file as speaker_diarization scores it (the
    purities are printed in path order).  Returns the list of (cls, purity_cluster_m, purity_speaker_m) in path order, each
    equal to speaker_diarization of that file.  n_speakers: an int or one per path; init_centers: None or one dict (or None)
    per path; a RandomState instance is consumed in PATH order, as the loop over the files would.  A file that cannot be read
    or served raises ValueError naming its index before the device is touched; what the data of a file makes the loop raise
    is raised after ALL batches have run and before any file is scored, named by the lowest such index: unlike the loop, no
    purity line of the files in front of it is printed then (speaker_diarization_evaluation(batch=True) prints none for that
    dimension).  A refusal of the arguments names the first file that fails within the first sampling-rate group that has one
    (groups in the order their rate first appears), which need not be the lowest index overall."""
    if lda_dim > 0:
        raise NotImplementedError(_LDA_ELSEWHERE)
    paths = list(paths)
    n = len(paths)
    if not n:
        return []
    loaded = _diar_models(models, models_dir)
    extra = _diar_extra_rows(loaded)
    groups, durations = {}, [0.0] * n
    for i, path in enumerate(paths):
        fs, sig = audioBasicIO.read_audio_file(path)
        if fs <= 0:
            raise ValueError("file %d (%s) cannot be read" % (i, path))
        mono = np.asarray(audioBasicIO.stereo_to_mono(sig))
        durations[i] = len(mono) / fs
        groups.setdefault(fs, []).append((i, mono))
    speakers = [int(n_speakers)] * n if np.ndim(n_speakers) == 0 else [int(s) for s in n_speakers]
    inits = [None] * n if init_centers is None else list(init_centers)
    if len(speakers) != n or len(inits) != n:
        raise ValueError("n_speakers and init_centers: one value per path (%d paths)" % n)
    windows, checked = [0] * n, [None] * n
    for fs, members in groups.items():
        ids = [i for i, _ in members]
        try:
            monos = _mono_clips([s for _, s in members])
            _, _, _, M = _diar_batch_plan([m.shape[0] for m in monos], fs, mid_window, mid_step)
            _, ks_list, group_inits = _diar_batch_check([2 * 68 + extra] * len(ids), M, [speakers[i] for i in ids], [inits[i] for i in ids])
        except ValueError as exc:
            raise _as_path_index(exc, ids)
        for j, i in enumerate(ids):
            windows[i], checked[i] = (int(M[j]), ks_list[j]), group_inits[j]
    draws = None
    if isinstance(random_state, np.random.RandomState):      # the loop consumes it file after file: draw in that order
        draws = [_diar_batch_draws(random_state, windows[i][0], windows[i][1], checked[i])[0] for i in range(n)]
    results = [None] * n
    for fs, members in groups.items():
        ids = [i for i, _ in members]
        out = _speaker_batch([s for _, s in members], fs, [speakers[i] for i in ids], mid_window, mid_step, loaded, random_state,
                             [inits[i] for i in ids], True, "record", chunk_bytes, None, None if draws is None else [draws[i] for i in ids])
        for i, r in zip(ids, out):
            results[i] = r
    for i, r in enumerate(results):
        if isinstance(r, BaseException):
            raise type(r)("clip %d: %s" % (i, r))
    return [_score_diarization(paths[i], results[i][0], results[i][1], mid_step, durations[i], speakers[i], plot_res) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------
# the LDA branch of speaker diarization (reference :880-934, :1001, :1012)
# ---------------------------------------------------------------------------------------------------------
LDA_TOL = 1e-4                                       # scikit-learn's LinearDiscriminantAnalysis(tol=1e-4)


def lda_window_labels(n_windows, short_window):
    """The class of every step-1 window as the reference computes it (:925-929): int(i * short_window / (1.0 / short_window)),
    in that floating-point form.  Labels never decrease."""
    lda_step_ratio = 1.0 / short_window
    return (np.arange(int(n_windows)) * short_window / lda_step_ratio).astype(np.int64)


def _lda_runs(labels, n):
    """Run boundaries [C + 1] of non-decreasing labels [n]."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("labels must hold one entry per window (%d)" % n)
    if n > 1 and np.any(labels[1:] < labels[:-1]):
        raise ValueError("labels decrease: only contiguous classes (non-decreasing labels, one run of windows per class) are "
                         "supported")
    starts = np.flatnonzero(np.concatenate(([True], labels[1:] != labels[:-1]))) if n else np.zeros(0, dtype=np.int64)
    return np.ascontiguousarray(np.concatenate((starts, [n])), dtype=np.int64)


def _lda_check(n_dims, n, offsets, n_components):
    n_classes = offsets.shape[0] - 1
    if n_dims < 1 or n_dims > _DIAR_MAX_DIMS or n < 1:
        raise ValueError("feature matrix of %d dims x %d windows: 1..%d dims and at least one window" % (n_dims, n, _DIAR_MAX_DIMS))
    if n_components < 1:
        raise ValueError("n_components must be at least 1")
    if n_components > min(n_dims, n_classes - 1):
        raise ValueError("n_components cannot be larger than min(n_features, n_classes - 1).")     # scikit-learn's message
    if n <= n_classes:
        raise ValueError("The number of samples must be more than the number of classes.")


def _eigh_desc(A):
    """Singular values and right singular vectors of a matrix from its Gram matrix A: sqrt of the eigenvalues (negative ones
    clamped to 0) in descending order, eigenvectors in the columns."""
    lam, V = np.linalg.eigh(A)
    order = np.argsort(lam)[::-1]
    return np.sqrt(np.maximum(lam[order], 0.0)), V[:, order]


def _margins(S, rank, threshold):
    kept = float(S[rank - 1] / threshold) if rank > 0 else 0.0
    dropped = float(threshold / S[rank]) if rank < S.shape[0] and S[rank] > 0 else np.inf
    return kept, dropped


def lda_fit_device(d_x, n_dims, ld, n, labels, n_components, tol=LDA_TOL):
    """LinearDiscriminantAnalysis(n_components, solver="svd", tol).fit of scikit-learn on a device matrix (DeviceBuffer of
    [n_dims][ld] doubles, window t in column t) with non-decreasing labels [n].  Class means, pooled within-class deviation
    and the Gram matrix G = Xs^T Xs of the centred, scaled windows come from the device (paa_lda_dev_*); the singular values
    and right singular vectors of Xs are those of G's eigen-decomposition (numpy.linalg.eigh, at most 256 x 256), and the
    same again for the Gram matrix of the weighted class means in the whitened space -- host work that does not grow with
    the number of windows.  Every column of scalings gets its largest-magnitude entry positive (an SVD leaves the sign
    open).  Returns a dict: xbar, means, priors, std, scalings [n_dims][min(n_components, rank2)], scalings_all, S, rank,
    S2, rank2, rank_margin / rank2_margin (kept / threshold, threshold / dropped), gram, offsets."""
    lib = _ffi.lib()
    offsets = _lda_runs(labels, n)
    _lda_check(n_dims, n, offsets, n_components)
    if ld < n:
        raise ValueError("bad feature matrix: %d vectors, ld %d" % (n, ld))
    n_classes = offsets.shape[0] - 1
    means, std = np.empty((n_classes, n_dims)), np.empty(n_dims)
    _ffi.check(lib.paa_lda_dev_class_stats_f64(d_x.ptr, n_dims, ld, n, _ffi.as_i64p(offsets), n_classes, _ffi.as_f64p(means),
                                               _ffi.as_f64p(std)))
    priors = np.diff(offsets) / float(n)
    xbar = priors @ means
    fac = 1.0 / (n - n_classes)
    G = np.empty((n_dims, n_dims))
    _ffi.check(lib.paa_lda_dev_within_gram_f64(d_x.ptr, n_dims, ld, n, _ffi.as_i64p(offsets), n_classes, _ffi.as_f64p(means),
                                               _ffi.as_f64p(std), fac, _ffi.as_f64p(G)))
    S, V = _eigh_desc(G)
    rank = int(np.sum(S > tol))
    if rank < 1:
        raise ValueError("the within-class scatter has no singular value above tol = %g" % tol)
    scalings = (V[:, :rank] / std[:, None]) / S[:rank]
    fac2 = 1.0 / (n_classes - 1)                                                  # _lda_check: at least two classes
    W = ((np.sqrt((n * priors) * fac2)) * (means - xbar).T).T @ scalings          # [C][rank]: the weighted class means
    S2, V2 = _eigh_desc(W.T @ W)
    rank2 = int(np.sum(S2 > tol * S2[0]))
    full = scalings @ V2[:, :rank2]
    top = np.argmax(np.abs(full), axis=0)
    full = full * np.where(full[top, np.arange(full.shape[1])] < 0, -1.0, 1.0)
    return {"xbar": xbar, "means": means, "priors": priors, "std": std, "gram": G, "offsets": offsets,
            "scalings": np.ascontiguousarray(full[:, :n_components]), "scalings_all": full, "S": S, "rank": rank, "S2": S2,
            "rank2": rank2, "rank_margin": _margins(S, rank, tol), "rank2_margin": _margins(S2, rank2, tol * S2[0]),
            "n_dims": n_dims, "tol": tol}


def lda_transform_device(model, d_x, n_dims, ld, n, d_y=None, ld_y=None):
    """(x - xbar) @ scalings of a fitted model for every window of a device matrix [n_dims][ld]: returns (d_y, n_out), the
    DeviceBuffer [n_out][ld_y] (made here when d_y is None, with ld_y = n; the caller frees it) -- the layout the
    clustering kernels read."""
    if n_dims != model["n_dims"]:
        raise ValueError("feature vectors have %d dims, the model %d" % (n_dims, model["n_dims"]))
    S = np.ascontiguousarray(model["scalings"], dtype=np.float64)
    n_out = S.shape[1]
    ld_y = n if ld_y is None else int(ld_y)
    if n < 1 or ld < n or ld_y < n:
        raise ValueError("bad feature matrix: %d vectors, ld %d, output ld %d" % (n, ld, ld_y))
    own = d_y is None
    if own:
        d_y = _ffi.DeviceBuffer(n_out * ld_y * 8)
    try:
        xbar = np.ascontiguousarray(model["xbar"], dtype=np.float64)
        _ffi.check(_ffi.lib().paa_lda_dev_project_f64(d_x.ptr, n_dims, ld, n, _ffi.as_f64p(xbar), _ffi.as_f64p(S), n_out, d_y.ptr,
                                                      ld_y))
    except BaseException:
        if own:
            d_y.free()
        raise
    return d_y, n_out


def lda_fit_transform(X, labels, n_components, *, tol=LDA_TOL, return_model=False):
    """LinearDiscriminantAnalysis(n_components).fit_transform(X, labels) for X (n_windows x n_dims) on the host, as
    scikit-learn takes it; the result is (n_windows x n_components), columns signed as lda_fit_device says.  ValueError --
    before any device work -- when n_components > min(n_dims, n_classes - 1) (scikit-learn's message), when there are not
    more windows than classes (scikit-learn divides by zero there), and when labels decrease: only contiguous classes are
    supported, which is what the reference's label formula produces."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be a (n_windows x n_dims) matrix")
    n, n_dims = X.shape
    _lda_check(n_dims, n, _lda_runs(labels, n), n_components)
    d_x = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(X.T))
    try:
        model = lda_fit_device(d_x, n_dims, n, n, labels, n_components, tol)
        d_y, n_out = lda_transform_device(model, d_x, n_dims, n, n)
        try:
            Y = d_y.to_host(np.float64, n_out * n).reshape(n_out, n).T.copy()
        finally:
            d_y.free()
    finally:
        d_x.free()
    return (Y, model) if return_model else Y


def speaker_diarization_lda_signal(signal, sampling_rate, n_speakers, mid_window=1.0, mid_step=0.1, short_window=0.1, lda_dim=35,
                                   *, models=None, models_dir=None, random_state=None, init_centers=None, return_details=False):
    """The LDA branch of speaker_diarization (reference :880-934, lda_dim > 0) on an array, resident on the device:

      mid-term statistics of the 68 short-term rows over int(round(mid_window / short_window)) frames at a step of ONE
      frame (one window per short-term frame, the last ones shorter); the probabilities of the two speaker SVMs + 1e-4
      below them; StandardScaler over the windows; labels int(i * short_window / (1.0 / short_window)); scikit-learn's
      LinearDiscriminantAnalysis(n_components=lda_dim).fit_transform (lda_fit_device); k-means for k = 2..9 (or
      n_speakers) and the silhouettes on the projection as it stands (cluster_prepared_device: no second
      standardisation, no dimension filter); a 5-tap median filter (zero-padded) over the labels of the LAST k tried.

    As in the reference the short-term window and step are round(fs * 0.05) whatever short_window says: short_window only
    enters the window ratio and the labels.  There is no HMM smoothing in this branch, mid_step is not used, and the result
    has one label per SHORT-TERM FRAME.  lda_dim > min(148, classes - 1) raises ValueError as scikit-learn does
    (lda_dim = 35 needs 36 classes).  init_centers: {k: [k][lda_dim]}.  With return_details: the dict of
    cluster_prepared_device plus "lda" (the model of lda_fit_device) and "lda_labels"."""
    from . import audioTrainTest
    if lda_dim <= 0:
        raise ValueError("lda_dim must be positive here: speaker_diarization_signal is the lda_dim = 0 form")
    loaded = _diar_models(models, models_dir)
    svcs = [(audioTrainTest.svc_model(m[0]), np.asarray(m[1], dtype=np.float64), np.asarray(m[2], dtype=np.float64)) for m in loaded]
    st = round(sampling_rate * 0.05)
    window_ratio = int(round(mid_window / short_window))
    if window_ratio < 1:
        raise ValueError("mid_window / short_window rounds to 0")
    rows, extra = 2 * 68, sum(len(s[0].classes) for s in svcs)
    n_dims = rows + extra
    lib = _ffi.lib()
    with _mid_term_on_device(audioBasicIO.stereo_to_mono(signal), sampling_rate, window_ratio * st / float(sampling_rate),
                             st / float(sampling_rate), st, st, extra) as (d_all, T):
        labels = lda_window_labels(T, short_window)
        _lda_check(n_dims, T, _lda_runs(labels, T), lda_dim)
        at = rows                                   # the probability rows go below the statistics
        for model, mean, std in svcs:
            _, proba = model.predict_device(d_all, T, T, mean, std)
            block = np.ascontiguousarray(proba.T + 1e-4)
            _ffi.check(lib.paa_memcpy_h2d(C.c_void_p(d_all.ptr.value + at * T * 8), block.ctypes.data_as(C.c_void_p), block.nbytes))
            at += block.shape[0]
        d_z = _ffi.DeviceBuffer(n_dims * T * 8)
        d_y = None
        try:
            stats = np.empty((3, n_dims))
            _ffi.check(lib.paa_diar_dev_standardize_f64(d_all.ptr, n_dims, T, T, d_z.ptr, _ffi.as_f64p(stats)))
            lda = lda_fit_device(d_z, n_dims, T, T, labels, lda_dim)
            d_y, n_out = lda_transform_device(lda, d_z, n_dims, T, T)
            details = cluster_prepared_device(d_y, n_out, T, n_speakers, random_state=random_state, init_centers=init_centers)
        finally:
            d_z.free()
            if d_y is not None:
                d_y.free()
    cls = median_filter5(details["labels"][details["ks"][-1]])              # the reference filters the LAST k's labels
    if return_details:
        details["lda"] = lda
        details["lda_labels"] = labels
        return cls, details
    return cls


def speaker_diarization_lda(filename, n_speakers, mid_window=1.0, mid_step=0.1, short_window=0.1, lda_dim=35, plot_res=False, *,
                            models=None, models_dir=None, random_state=None, init_centers=None):
    """speaker_diarization(filename, ..., lda_dim > 0) of the reference: returns (cls, purity_cluster_m, purity_speaker_m) --
    one label per short-term frame (float64, see speaker_diarization_lda_signal) and the purities against
    <filename>.segments when it exists, else -1, -1.  As in the reference the ground truth is sampled -- and the plot's time
    axis drawn -- at mid_step although the labels step by 0.05 s.  models, random_state, init_centers: see
    speaker_diarization."""
    loaded = _diar_models(models, models_dir)
    sampling_rate, signal = audioBasicIO.read_audio_file(filename)
    signal = audioBasicIO.stereo_to_mono(signal)
    duration = len(signal) / sampling_rate
    cls, details = speaker_diarization_lda_signal(signal, sampling_rate, n_speakers, mid_window, mid_step, short_window, lda_dim,
                                                  models=loaded, random_state=random_state, init_centers=init_centers,
                                                  return_details=True)
    return _score_diarization(filename, cls, details, mid_step, duration, n_speakers, plot_res)
