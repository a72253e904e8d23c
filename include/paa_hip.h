/*
 * paa_hip.h -- C ABI of libpaa_hip.so, the MI355X (gfx950) short-term / mid-term audio
 * feature extractor that is a drop-in for ONE path of tyiannak/pyAudioAnalysis.
 *
 * The reference has no FFI layer: its boundary is the Python signature.  Each entry point
 * below names the reference interface it replaces (paths relative to
 * /root/reference/pyAudioAnalysis).  Plain pointers and sizes only; no torch / numpy types.
 * INTEGRATION.md shows the ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - return value 0 (PAA_OK) = success, < 0 = error code; paa_last_error() gives the text
 *     (thread local).  There is NO CPU fallback: without a HIP device every compute call
 *     returns PAA_ERR_HIP.
 *   - `window` / `step` are in samples and already int()-truncated by the caller
 *     (ShortTermFeatures.py:563-564); num_fft = window / 2 (integer division, :575).
 *   - host buffers are caller-owned and only touched during the call.  `*_dev_*` entry points
 *     take HIP device pointers (from paa_dev_alloc or any hipMalloc) and are asynchronous on
 *     the library's stream; paa_dev_sync() waits for them.
 *   - feature matrices are float64, C-contiguous, FEATURE-major [F][T] (F = 34, or 68 with
 *     deltas), exactly the reference's return layout (:684); spectrogram / chromagram are
 *     TIME-major [T'][num_fft] / [T''][12] (:413, :347).
 *   - a batch is a packed sample buffer plus n_clips+1 sample offsets; clip c's result is the
 *     [F][T_c] slab starting at out + out_offsets[c] (in doubles).
 */
#ifndef PAA_HIP_H
#define PAA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAA_OK                 0
#define PAA_ERR_ARG          (-1)  /* bad argument (null pointer, window < 2, step < 1, ...)          */
#define PAA_ERR_UNSUPPORTED  (-2)  /* window beyond the LDS envelope of the kernels                    */
#define PAA_ERR_HIP          (-3)  /* HIP runtime error / no device                                    */
#define PAA_ERR_OOM          (-4)  /* device or host allocation failed                                 */
#define PAA_ERR_TOO_SHORT    (-5)  /* fewer samples than one window: reference raises ValueError :684  */
#define PAA_ERR_CHROMA_VALUE (-6)  /* chroma slot > num_fft: reference raises ValueError :293          */
#define PAA_ERR_CHROMA_INDEX (-7)  /* chroma slot == num_fft: reference raises IndexError :291         */
#define PAA_ERR_MEL_INDEX    (-8)  /* mel filter bin >= num_fft: reference raises IndexError :230-231  */
#define PAA_ERR_COMM         (-9)  /* RCCL error                                                       */

#define PAA_N_BASE_FEATURES 34

/* ---- library / device management ------------------------------------------------------ */
const char *paa_version(void);
const char *paa_last_error(void);
int  paa_device_count(void);             /* >= 0, or PAA_ERR_HIP                                   */
int  paa_init(int device_id);            /* select the device for this process (one process per GPU) */
void paa_shutdown(void);                 /* free cached tables, scratch and the stream              */
/* PCI bus id of the selected device ("0000:75:00.0", NUL-terminated): names the physical device whatever
 * HIP_VISIBLE_DEVICES says; used to refuse two ranks of one RCCL job on one device                  */
int  paa_device_bus_id(char *out, int capacity);
int  paa_dev_alloc(size_t bytes, void **out_ptr);
int  paa_dev_free(void *ptr);
int  paa_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);   /* synchronous */
int  paa_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes);    /* queued on the library stream */
int  paa_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);   /* synchronous */
/* the same, ordered behind the kernels of the compute stream only -- not behind gathers still queued on the communication
 * stream.  For buffers that are at most the SOURCE of a gather (distributed.py's restart shards are saved with it while the
 * exchange may still be waiting for a peer); a gather DESTINATION must be read with paa_memcpy_d2h                    */
int  paa_memcpy_d2h_compute(void *dst_host, const void *src_dev, size_t bytes);
int  paa_dev_sync(void);
/* elapsed GPU milliseconds between two points of the library stream (HIP events) */
int  paa_timer_start(void);
int  paa_timer_stop(float *ms);

/* HIP-event timing of the feature kernel inside paa_plan_execute (off by default): every_nth = 1 brackets every
 * launch with an event pair, n > 1 every n-th one (an event pair is an ordering point on the stream, so the
 * recorder itself slows a stream of back-to-back launches by ~4 % at n = 1), 0 switches it off;
 * paa_prof_read returns the accumulated milliseconds / number of timed launches and resets them */
int  paa_prof_enable(int every_nth);
int  paa_prof_read(double *total_ms, int64_t *launches);

/* ---- shape helpers ----------------------------------------------------------------------- */
/* T = floor((n - window)/step) + 1, 0 if n < window            (ShortTermFeatures.py:608)   */
int64_t paa_num_frames(int64_t n_samples, int window, int step);
/* M = ceil(T / mid_step_ratio)                                  (MidTermFeatures.py:116-124) */
int64_t paa_num_mid_windows(int64_t n_frames, int64_t mid_step_ratio);
/* rows allocated by spectrogram: int((n-window)/step)+1; rows actually filled in *filled     */
int64_t paa_spectrogram_rows(int64_t n_samples, int window, int step, int64_t *filled);
/* rows allocated by chromagram: int((n-step-window)/step)+1; filled rows in *filled          */
int64_t paa_chromagram_rows(int64_t n_samples, int window, int step, int64_t *filled);

/* ---- ShortTermFeatures.feature_extraction (ShortTermFeatures.py:543-685) ---------------- */
/* signal: int16 PCM as scipy.io.wavfile returns it (audioBasicIO.py:99), or float64
 * (after stereo_to_mono, audioBasicIO.py:167).  Both are scaled by 1/2^15 (:568).
 * out: [F][T] doubles, F = 34 * (deltas ? 2 : 1).                                         */
int paa_st_features_i16(const int16_t *signal, int64_t n, double fs, int window, int step,
                        int deltas, double *out);
int paa_st_features_f64(const double *signal, int64_t n, double fs, int window, int step,
                        int deltas, double *out);

/* interleaved stereo int16 (L0 R0 L1 R1 ..., n frames): audioBasicIO.stereo_to_mono (audioBasicIO.py:156-168) is
 * fused into the kernels' sample loads (L + R summed exactly as it is fetched, scaled by 2^-16): the mono signal is
 * never materialised; stereo files cost 4 B/sample over PCIe and HBM instead of the 8 B of the float64 mono copy the
 * reference makes on the host                                                                              */
int paa_st_features_stereo_i16(const int16_t *interleaved, int64_t n, double fs, int window, int step,
                               int deltas, double *out);
int paa_mid_features_stereo_i16(const int16_t *interleaved, int64_t n, double fs, int window, int step,
                                int64_t mid_ratio, int64_t mid_step_ratio, double *mid_out, double *st_out);

/* ---- MidTermFeatures.mid_feature_extraction (MidTermFeatures.py:87-127) ----------------- */
/* mid_ratio / mid_step_ratio are computed by the caller with Python round() (:100-102).  Any mid_ratio is accepted:
 * window m is row[m*step : min(m*step + mid_ratio, T)] with Python's slice rules (a negative end counts from the row's end).
 * st_out: [68][T] (deltas always on, :93-95), may be NULL; mid_out: [136][M].               */
int paa_mid_features_i16(const int16_t *signal, int64_t n, double fs, int window, int step,
                         int64_t mid_ratio, int64_t mid_step_ratio, double *mid_out, double *st_out);
int paa_mid_features_f64(const double *signal, int64_t n, double fs, int window, int step,
                         int64_t mid_ratio, int64_t mid_step_ratio, double *mid_out, double *st_out);

/* ---- ShortTermFeatures.spectrogram / chromagram (:389-452 / :324-386) ------------------- */
/* out has paa_spectrogram_rows() x (window/2) doubles; unfilled trailing rows are zeroed.   */
int paa_spectrogram_i16(const int16_t *signal, int64_t n, double fs, int window, int step, double *out);
int paa_spectrogram_f64(const double *signal, int64_t n, double fs, int window, int step, double *out);
/* out has paa_chromagram_rows() x 12 doubles.  The reference may FFT a truncated last frame
 * (:349-355); that frame is evaluated on the device as a direct DFT of its true length.      */
int paa_chromagram_i16(const int16_t *signal, int64_t n, double fs, int window, int step, double *out);
int paa_chromagram_f64(const double *signal, int64_t n, double fs, int window, int step, double *out);
/* interleaved stereo int16 (n frames): audioAnalysis.fileSpectrogramWrapper / fileChromagramWrapper call stereo_to_mono
 * first (audioAnalysis.py:66-81, audioBasicIO.py:156-168); here the channels are summed on the device (4 B/frame over PCIe
 * instead of the 8 B of the float64 mono copy)                                                                  */
int paa_spectrogram_stereo_i16(const int16_t *interleaved, int64_t n, double fs, int window, int step, double *out);
int paa_chromagram_stereo_i16(const int16_t *interleaved, int64_t n, double fs, int window, int step, double *out);

/* ---- batched many-clip path (what MidTermFeatures.directory_feature_extraction :140-221
 *      does sequentially per file)                                                          */
int paa_st_features_batch_i16(const int16_t *packed, const int64_t *offsets, int64_t n_clips,
                              double fs, int window, int step, int deltas,
                              double *out, const int64_t *out_offsets);
/* float64 clips (what stereo_to_mono / np.double() hand the reference for stereo, 8-bit, 32-bit or float files,
 * audioBasicIO.py:167, ShortTermFeatures.py:567): the same batch, 8 B/sample                 */
int paa_st_features_batch_f64(const double *packed, const int64_t *offsets, int64_t n_clips,
                              double fs, int window, int step, int deltas,
                              double *out, const int64_t *out_offsets);
int paa_mid_features_batch_f64(const double *packed, const int64_t *offsets, int64_t n_clips,
                               double fs, int window, int step,
                               int64_t mid_ratio, int64_t mid_step_ratio,
                               double *mid_out, const int64_t *mid_out_offsets,
                               double *st_out, const int64_t *st_out_offsets);
/* mid_out_offsets index [136][M_c] slabs; st_out / st_out_offsets may be NULL               */
int paa_mid_features_batch_i16(const int16_t *packed, const int64_t *offsets, int64_t n_clips,
                               double fs, int window, int step,
                               int64_t mid_ratio, int64_t mid_step_ratio,
                               double *mid_out, const int64_t *mid_out_offsets,
                               double *st_out, const int64_t *st_out_offsets);

/* ---- device-resident plans (bench / pipelines: samples and results stay in HBM) --------- */
typedef struct paa_plan paa_plan_t;
/* offsets: n_clips+1 HOST sample offsets into the packed device buffer.  sample_kind 0 = int16,
 * 1 = float64, 2 = interleaved stereo int16 (offsets count stereo frames of 4 bytes; L + R is formed in the kernels'
 * loads and scaled by 2^-16 = stereo_to_mono followed by :568).  The plan owns the tables, the tile list and the
 * per-clip statistics.                                                                                      */
int paa_plan_create(const int64_t *offsets, int64_t n_clips, int sample_kind, double fs,
                    int window, int step, int deltas, paa_plan_t **out_plan);
/* spectrogram (mode 1) / chromagram (mode 2) rows kept in HBM (ShortTermFeatures.py:389-452, :324-386); mode 0 = features
 * without deltas.  paa_plan_out_doubles() gives the size of the row block, paa_plan_total_frames() the full-length frames. */
int paa_plan_create_mode(const int64_t *offsets, int64_t n_clips, int sample_kind, double fs, int window, int step,
                         int mode, paa_plan_t **out_plan);
int paa_plan_destroy(paa_plan_t *plan);
int64_t paa_plan_total_frames(const paa_plan_t *plan);
int64_t paa_plan_out_doubles(const paa_plan_t *plan);     /* sum_c F*T_c                      */
/* out_offsets (HOST, n_clips) receives the slab start of every clip when non-NULL           */
int paa_plan_out_offsets(const paa_plan_t *plan, int64_t *out_offsets);
/* asynchronous on the library stream: clip statistics -> features (+deltas) into d_out       */
int paa_plan_execute(paa_plan_t *plan, const void *d_packed, double *d_out);
/* optional mid-term statistics of an executed plan (deltas must be on): d_mid gets
 * [136][M_c] slabs back to back; returns total doubles via paa_plan_mid_doubles             */
int64_t paa_plan_mid_doubles(const paa_plan_t *plan, int64_t mid_step_ratio);
int paa_plan_mid_execute(paa_plan_t *plan, const double *d_st, int64_t mid_ratio,
                         int64_t mid_step_ratio, double *d_mid);
/* MidTermFeatures.beat_extraction (MidTermFeatures.py:18-84) for every clip of an executed plan:
 * d_beat receives [n_clips][2] = (bpm, confidence); window_size = short-term step in seconds.
 * The histogram has round(2 / window_size) bins.  No bins (window_size >= 4 s) -> PAA_ERR_ARG (the reference raises
 * ValueError).  One workgroup holds every row's histogram in LDS next to its frame tile:
 * 18 * 129 * 8 + 18 * 4 * bins bytes, at most the 160 KB of a gfx950 workgroup, i.e. at most 2 017 bins (a step longer
 * than about 0.9913 ms).  More bins -> PAA_ERR_UNSUPPORTED; this limit is the library's own, the reference has none. */
int paa_plan_beat_execute(paa_plan_t *plan, const double *d_st, double window_size, double *d_beat);
/* the same (same limits) for ONE short-term matrix in host memory (the reference's own signature, MidTermFeatures.py:18): feats is
 * [n_rows][n_frames] feature-major (n_rows >= 19: rows 0..18 are read, :30-31); bpm_ratio receives (bpm, confidence) */
int paa_beat_extraction_f64(const double *feats, int n_rows, int64_t n_frames, double window_size, double *bpm_ratio);
/* name of the feature kernel the plan dispatches ("st_fast_800", "st_generic", ...)          */
const char *paa_plan_kernel_name(const paa_plan_t *plan);

/* delta rows re-formed on the device (ShortTermFeatures.py:668-680): d_base holds the [34][T_c] base-feature slabs of
 * n_clips clips back to back (frames[c] = T_c, HOST array), d_out receives their [68][T_c] slabs back to back -- rows
 * 34..67 are the differences of consecutive columns, column 0 zeros, bit-identical to what a 68-row plan stores.  A sharded
 * job gathers the 34 base rows over xGMI and the root completes the matrices (half the bytes on the links).  Asynchronous:
 * queued behind the gathers on the communication stream when a communicator exists, else on the library stream          */
int paa_dev_expand_deltas(const double *d_base, const int64_t *frames, int64_t n_clips, double *d_out);

/* ---- self-similarity matrix / music thumbnailing ----------------------------- */
/* audioSegmentation.self_similarity_matrix (audioSegmentation.py:40-55): rows standardised like scikit-learn's
 * StandardScaler, sim[i][j] = 1 - cosine distance of columns i, j (SciPy pdist semantics: clipped cosine, exact 1
 * on the diagonal, NaN for zero vectors).  feats is [n_dims][n_vec] row-major -- the layout feature_extraction
 * returns; sim is [n_vec][n_vec].  Host buffers:                                                */
int paa_self_similarity_f64(const double *feats, int n_dims, int64_t n_vec, double *sim);
/* the same on device buffers (asynchronous on the library stream); ld = row pitch of d_feats in doubles, so the
 * output of paa_plan_execute for a one-clip plan can be passed as is                            */
int paa_dev_self_similarity(const double *d_feats, int n_dims, int64_t n_vec, int64_t ld, double *d_sim);
/* matrix part of audioSegmentation.music_thumbnailing (:1141-1165): moving sum of m_filter cells along the
 * diagonals (convolve2d with eye(m_filter), 'valid'), cells with |i-j| < band, i > j or outside
 * [int(limit_1 R), int(limit_2 R)) set to the global minimum, then the arg-max (first maximum in row-major
 * order).  R = paa_thumbnail_rows(n_vec, m_filter) = n_vec - m_filter + 1; filt is [R][R]; pos2 (HOST) receives
 * (row, column).  n_vec < m_filter is rejected with PAA_ERR_ARG.                                */
int64_t paa_thumbnail_rows(int64_t n_vec, int m_filter);
int paa_thumbnail_f64(const double *feats, int n_dims, int64_t n_vec, int m_filter, double band, double limit_1,
                      double limit_2, double *filt, int64_t *pos2);
/* device buffers in and out; synchronises the library stream before returning pos2.  d_sim must be symmetric bit for
 * bit, as paa_dev_self_similarity writes it: the diagonal sums are formed for j >= i only (the cells below the
 * diagonal are masked, and the minimum over one triangle is the minimum over the matrix)       */
int paa_dev_thumbnail_filter(const double *d_sim, int64_t n_vec, int m_filter, double band, double limit_1,
                             double limit_2, double *d_filt, int64_t *pos2);

/* ---- music thumbnailing for a batch of clips ------------------------------------------------
 * The stages above for n_clips RAGGED clips in one call: clip c has n_vec[c] vectors and R_c = n_vec[c] - m_filter + 1
 * filtered rows; the Gram tiles, the diagonal blocks and the folds of all clips are one launch each, and the arg-max cell is
 * grown on the device (audioSegmentation.py:1167-1182).  Clip c of any batch gets the bits of its own single call
 * (paa_self_similarity_f64, paa_thumbnail_f64, paa_dev_thumbnail_filter), at any position, beside any other clips, under
 * any chunk_bytes.  pos is [n_clips][2] (row, column of the arg-max), bounds [n_clips][4] = (i1, i2, j1, j2): the two
 * thumbnail instances in vectors.  Refused before the device is touched: null buffers, n_clips < 1, n_dims < 1, negative
 * or NaN limits, a clip with n_vec < m_filter (PAA_ERR_ARG) or past paa_dev_self_similarity's size bound
 * (PAA_ERR_UNSUPPORTED); the message names the clip.
 * Host buffers, packed clip after clip: feats holds the [n_dims][n_vec[c]] row-major matrices, sims / sim the
 * n_vec[c] x n_vec[c] matrices, filt (may be null) the R_c x R_c matrices.  Whole clips are taken in chunks whose device
 * scratch (Z, both matrices, candidates, lists) stays within chunk_bytes (0: 1 GiB, the bound for larger values too); a
 * clip that alone needs more is a chunk of its own; no result depends on it.                         */
int paa_self_similarity_batch_f64(const double *feats, int n_dims, int64_t n_clips, const int64_t *n_vec, int64_t chunk_bytes,
                                  double *sim);
int paa_thumbnail_filter_batch_f64(const double *sims, int64_t n_clips, const int64_t *n_vec, int m_filter, double band,
                                   double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos, int64_t *bounds, double *filt);
int paa_thumbnail_batch_f64(const double *feats, int n_dims, int64_t n_clips, const int64_t *n_vec, int m_filter, double band,
                            double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos, int64_t *bounds, double *filt);
/* end to end: packed samples (clip c = [offsets[c], offsets[c + 1]), ascending) -> ONE plan per chunk with 68 rows -> the
 * stages on the plan's slabs in HBM; only pos, bounds and -- when filt is given -- the filtered matrices come back.  A
 * clip shorter than one window is PAA_ERR_ARG as well.                                               */
int paa_music_thumbnail_batch_i16(const int16_t *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                                  int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos,
                                  int64_t *bounds, double *filt);
int paa_music_thumbnail_batch_f64(const double *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                                  int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos,
                                  int64_t *bounds, double *filt);
/* the same with one HOST pointer per clip in place of the packed array (offsets still give the lengths): clips that sit in
 * memory one by one go to the device without being copied together first                              */
int paa_music_thumbnail_batch_ptrs_i16(const int16_t *const *clips, const int64_t *offsets, int64_t n_clips, double fs, int window,
                                       int step, int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes,
                                       int64_t *pos, int64_t *bounds, double *filt);
int paa_music_thumbnail_batch_ptrs_f64(const double *const *clips, const int64_t *offsets, int64_t n_clips, double fs, int window,
                                       int step, int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes,
                                       int64_t *pos, int64_t *bounds, double *filt);
/* the two stages on device buffers; offsets (in doubles) and counts are HOST int64 arrays [n_clips].  Asynchronous on the
 * library stream, no synchronisation inside: d_pos [n_clips][2] and d_bounds [n_clips][4] are DEVICE int64 arrays.  ld[c]
 * is the row pitch of clip c's matrix, so the slabs of a batched plan can be passed as they are.     */
int paa_dev_self_similarity_batch(const double *d_feats, int n_dims, int64_t n_clips, const int64_t *feat_off,
                                  const int64_t *n_vec, const int64_t *ld, double *d_sim, const int64_t *sim_off);
int paa_dev_thumbnail_filter_batch(const double *d_sim, const int64_t *sim_off, const int64_t *n_vec, int64_t n_clips,
                                   int m_filter, double band, double limit_1, double limit_2, double *d_filt,
                                   const int64_t *filt_off, int64_t *d_pos, int64_t *d_bounds);
/* host only (tests): the layout a batch of these clips gets.  counts [3] = Gram tiles, diagonal blocks, fill row blocks;
 * tiles / blocks / rows [cap][3] = (clip, ti, tj) / (clip, bx, by) / (clip, 0, by); clip_off [n_clips][3] = the clip's
 * offsets into the Z, norm and candidate scratch                                                     */
int paa_debug_thumbnail_batch_layout(const int64_t *n_vec, int64_t n_clips, int n_dims, int m_filter, int64_t *counts,
                                     int32_t *tiles, int64_t tiles_cap, int32_t *blocks, int64_t blocks_cap, int32_t *rows,
                                     int64_t rows_cap, int64_t *clip_off);

/* ---- silence_removal's per-frame SVM loop (audioSegmentation.py:744-748) ------------------------------
 * P(class index 1) of a TRAINED binary probabilistic scikit-learn SVC for every column of feats [n_dims][n_frames]
 * (host, feature-major like the short-term matrix): (x - mean) / scale (:746), decision value from the support vectors
 * (support_vectors [n_sv][n_dims], dual_coef [n_sv], intercept; gamma > 0: RBF kernel, gamma <= 0: linear), Platt
 * sigmoid with (prob_a, prob_b) and libsvm's two-class multiclass_probability -- svm.predict_proba(..)[0][1] per frame.
 * Training (:739) stays with scikit-learn.                                                                  */
int paa_svm_binary_proba_f64(const double *feats, int n_dims, int64_t n_frames, const double *mean, const double *scale,
                             const double *support_vectors, const double *dual_coef, int n_sv, double intercept,
                             double gamma, double prob_a, double prob_b, double *prob1);

/* ---- audioTrainTest.classifier_wrapper for SVM models (audioTrainTest.py:84-93) --------------------------------------
 * predict() and predict_proba() of a TRAINED multi-class probabilistic scikit-learn SVC (SVC(probability=True), kernel
 * 'rbf' or 'linear') for many feature vectors at once: what mid_term_file_classification (audioSegmentation.py:583-594) and
 * file_classification (audioTrainTest.py:1091-1095) ask for once per vector.  The model is libsvm's as scikit-learn holds
 * it: support_vectors [n_sv][n_dims] grouped by class, n_support [n_classes], dual_coef [n_classes - 1][n_sv] (libsvm's
 * sv_coef = scikit-learn's _dual_coef_), rho / prob_a / prob_b [n_classes (n_classes - 1) / 2] (rho = -_intercept_),
 * kernel_type 0 (LINEAR) or 2 (RBF, with gamma = _gamma).  2 <= n_classes <= 16, n_dims <= 256: anything else returns
 * PAA_ERR_ARG.  The model is uploaded once (paa_svc_create) and stays on the device until paa_svc_destroy.
 * feats is feature-major [n_dims][ld] (the mid-term matrix layout), vector v in column v; each is standardised on load,
 * (x - mean) / std (audioSegmentation.py:586).  label_index [n_vec] receives libsvm's vote winner (first maximum; the
 * caller maps it through classes_), proba [n_vec][n_classes] predict_proba's row.                                    */
int paa_svc_create(const double *support_vectors, int n_sv, int n_dims, const int32_t *n_support, int n_classes,
                   const double *dual_coef, const double *rho, const double *prob_a, const double *prob_b, int kernel_type,
                   double gamma, void **out_handle);
int paa_svc_destroy(void *handle);
int paa_svc_num_classes(const void *handle);
/* host buffers in and out (synchronous) */
int paa_svc_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec, const double *mean,
                        const double *std, int32_t *label_index, double *proba);
/* device buffers in and out (the resident mid-term matrix of a plan, paa_plan_mid_execute), asynchronous on the library
 * stream; at most one of these is in flight per process (they share a scratch buffer, in stream order)                */
int paa_svc_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                            const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba);

/* ---- audioTrainTest.Knn.classify for the kNN models (audioTrainTest.py:33-49) -------------------------------------------
 * k-nearest-neighbour classification of many feature vectors at once: what mid_term_file_classification
 * (audioSegmentation.py:583-594) and file_classification (audioTrainTest.py:1091-1095) ask for once per vector with a
 * knn_* model.  The model: train [n_train][n_dims], labels [n_train] (the class INDEX of every row; a value outside
 * 0..n_classes-1 votes for no class), n_classes = the number of distinct labels, k = `neighbors`.  1 <= k <= 32,
 * 1 <= n_classes <= 64, 1 <= n_dims <= 256: anything else returns PAA_ERR_ARG.  Uploaded once (paa_knn_create), on the
 * device until paa_knn_destroy.
 * feats is feature-major [n_dims][ld], vector v in column v, standardised on load, (x - mean) / std.  Neighbours are ranked
 * by the squared Euclidean distance sum_d (t_d - x_d)^2, ties by the training index (ascending (d^2, index)).
 * label_index [n_vec] receives the first class with the most votes, proba [n_vec][n_classes] P[c] = votes(c) / k (as in
 * the reference, also when n_train < k), neighbors [n_vec][k] (may be NULL) the neighbour indices in that order, -1 where
 * n_train < k.  A vector with NaN distances (a NaN query) gets no neighbours: P = 0, label 0.                          */
int paa_knn_create(const double *train, const int32_t *labels, int n_train, int n_dims, int n_classes, int k,
                   void **out_handle);
int paa_knn_destroy(void *handle);
int paa_knn_num_classes(const void *handle);
/* host buffers in and out (synchronous) */
int paa_knn_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec, const double *mean,
                        const double *std, int32_t *label_index, double *proba, int32_t *neighbors);
/* device buffers in and out (the resident mid-term matrix of a plan, paa_plan_mid_execute), asynchronous on the library
 * stream                                                                                                              */
int paa_knn_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                            const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba,
                            int32_t *d_neighbors);

/* ---- the kNN half of audioTrainTest.evaluate_classifier (audioTrainTest.py:631-700) ----------------------------------------
 * evaluate_classifier draws len(params) x n_exp random splits of one sample matrix and, for "knn", runs Knn.classify
 * (:33-49) once per test vector of every split after a StandardScaler fitted on that split's training rows (:652-680).  Here
 * every split is a JOB of two index lists over ONE sample matrix, and all jobs run in one launch; X is uploaded once per call.
 *   X [n_samples][n_dims]    every sample, row-major (1 <= n_dims <= 256, 1 <= n_samples < 2^31)
 *   labels [n_samples]       the class INDEX of every sample; -1 (any value outside 0..n_classes[j]-1) votes for no class
 *   n_jobs >= 1              number of jobs
 *   train_off [n_jobs + 1], train_idx [train_off[n_jobs]]   job j trains on the samples train_idx[train_off[j] .. train_off[j+1]-1],
 *                            in that order (the rows of the reference's X_train); at least one per job
 *   test_off [n_jobs + 1], test_idx [test_off[n_jobs]]      ... and classifies the samples test_idx[test_off[j] .. test_off[j+1]-1];
 *                            an empty test list is legal.  Offsets begin at 0 and do not decrease; indices are 0..n_samples-1;
 *                            lists may repeat and overlap
 *   mean, std [n_jobs][n_dims]   job j's standardisation: every training and test row is (x - mean_j) / std_j, IEEE division,
 *                            element by element BEFORE the difference is taken (StandardScaler.transform, :658, :676)
 *   k [n_jobs]               1 <= k[j] <= 32 (Knn.neighbors of the split)
 *   n_classes [n_jobs]       1 <= n_classes[j] <= max_classes <= 64: the number of distinct training labels of the split
 *                            (Knn.classify :40 counts them per split: a class absent from it shrinks n_classes, and rows labelled
 *                            >= n_classes[j] vote for no class)
 * Neighbours are ranked in ascending (d^2, position in the job's train list), d^2 = sum_d (t_d - x_d)^2 of the standardised
 * rows: the tie rule is the row index into the reference's X_train, NOT the sample index.  The first k[j] of that order vote.
 * Outputs hold Q = test_off[n_jobs] rows, in job order then test-list order:
 *   label_out [Q]            the first class < n_classes[j] with the most votes
 *   proba_out [Q][max_classes]   (may be NULL) votes(c) / k[j], also when the job has fewer than k[j] rows; 0 at c >= n_classes[j]
 *   neighbors_out [Q][K]     (may be NULL) the neighbours' train-list positions in that order, -1 past k[j] or past the train list;
 *                            K = the smallest of 1, 2, 4, 8, 16, 32 that is >= max_j k[j] (the kernel instance the sweep runs at)
 * A query with NaN distances (std 0 where x == mean) gets no neighbours: P = 0, label 0; other jobs are unaffected.
 * PAA_ERR_ARG, with a message and before the device is touched: a null pointer (other than the two optional outputs), offsets
 * that do not begin at 0 or decrease, an index outside 0..n_samples-1, k / classes / dims outside the limits above, an empty
 * train list, Q > 2^31 - 1.  Q == 0 returns PAA_OK and writes nothing.  Synchronous, host buffers in and out.
 * Of evaluate_classifier's six classifier types only "knn" is served here; the five scikit-learn types keep scikit-learn's
 * fits and gain only one paa_svc_* / paa_forest_* launch per fitted model in place of the per-vector predict loop, and SMOTE
 * resampling (smote=True, :653-656) is refused by the Python layer: its rows are no rows of X.                           */
int paa_knn_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                       const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx,
                       const double *mean, const double *std, const int32_t *k, const int32_t *n_classes, int max_classes,
                       int32_t *label_out, double *proba_out, int32_t *neighbors_out);
/* tests: out10 = queries per workgroup, training rows per LDS tile, rows per step, the number of K instances, the instances */
int paa_debug_knn_split_geometry(int32_t *out10);

/* ---- the SVM half of audioTrainTest.evaluate_classifier (audioTrainTest.py:631-700 with train_svm :132-155) ---------------------
 * For "svm" / "svm_rbf" evaluate_classifier fits sklearn.svm.SVC(C, kernel, probability=True, gamma='auto') once per split and reads
 * only the vote labels of predict(); libsvm fits every pair of classes (svm.cpp: svm_train -> svm_train_one -> solve_c_svc ->
 * Solver::Solve), and with probability=True five more times per pair for Platt's cross-validation, which the sweep never reads.
 * Here a TASK is one binary C-SVC dual problem over rows of ONE resident sample matrix, one workgroup solves one task with
 * libsvm's Solver without shrinking in FP64 throughout (libsvm keeps its kernel cache in float32, so agreement with scikit-learn is
 * bounded by the stopping tolerance, not bit-exact), and all tasks of a call run side by side.
 *
 * paa_smo_tasks_f64 -- the solver alone (Solver::Solve, select_working_set, calculate_rho):
 *   X [n_samples][n_dims]    every sample, row-major (1 <= n_dims <= 256, 1 <= n_samples < 2^31)
 *   task_off [n_tasks + 1], task_idx / task_sign [task_off[n_tasks]]   task t owns the rows task_idx[task_off[t] .. task_off[t+1]-1]
 *                            of X with the signs task_sign[..] (+1: the first class of the pair, -1: the second); 1..8192 rows
 *   mean, std [n_tasks][n_dims]   task t's standardisation, (x - mean_t) / std_t with an IEEE division on the load path
 *   C, gamma [n_tasks]       C > 0; gamma > 0 is read for kernel_type 2 only
 *   kernel_type              0: K = z_t . z_s;  2: K = exp(-gamma |z_t - z_s|^2)  (libsvm's LINEAR / RBF)
 *   eps > 0                  stop when Gmax + Gmax2 < eps (SVC's tol);  max_iter >= 1 (libsvm's floor is 10^7)
 *   iters_per_launch         iterations a task may run in one kernel launch (0: the default, 1024); the state lives in device
 *                            memory between launches, the host compacts the unfinished tasks and launches again.  No launch is
 *                            unbounded, and every output is bit-identical for any value, for a task alone or in any batch
 * Outputs: alpha_y [task_off[n_tasks]] = alpha_t y_t; per task rho, iterations, gap (the last Gmax + Gmax2; 0 when an index set was
 * empty) and status (2: converged, 3: max_iter reached -- outputs are those of the last iterate, finite); n_launches may be NULL.
 * The decision value of a standardised z is sum_t alpha_t y_t K(z_t, z) - rho; positive votes for the first class.
 *
 * paa_svc_fit_splits_f64 -- the sweep, in the job form of paa_knn_splits_f64 (labels, train_off / train_idx, test_off / test_idx,
 * mean / std [n_jobs][n_dims]) plus C, gamma [n_jobs].  The host builds job j's tasks from the classes PRESENT in its training
 * list in ascending order: per pair (a, b), a < b, row-major, the rows of a in train-list order, then those of b.  Every test
 * row gets the decision value of each pair over the task's rows with alpha != 0, libsvm's vote (dec > 0: a, else b) and the
 * first class with the most votes.
 *   label_out [Q]            the class INDEX (a value of `labels`), Q = test_off[n_jobs] rows in job order then test-list order
 *   dec_out [Q][max_pairs]   (may be NULL) the decision values, zeros past a job's pairs; max_pairs >= every job's pair count
 *   task_iterations, task_status, task_n_sv [n_tasks]   (each may be NULL) per task in job order then pair order; n_tasks must then
 *                            equal the number of tasks the jobs make;  n_launches (may be NULL)
 * PAA_ERR_ARG, with a message and before the device is touched: a null pointer (other than the optional outputs), offsets that do
 * not begin at 0 or decrease, an index outside 0..n_samples-1, a sign other than +-1, a negative training label, n_dims < 1,
 * C <= 0, gamma <= 0 (RBF), eps <= 0, kernel_type other than 0 / 2, max_iter < 1, an empty task, a job whose training list holds
 * fewer than two classes.  PAA_ERR_UNSUPPORTED, likewise before the device is touched: n_dims > 256 (PAA_SMO_MAX_DIMS), a task of
 * more than 8192 rows (PAA_SMO_MAX_ROWS), a job with more than 64 classes.  An empty test list is legal.  Synchronous, host
 * buffers in and out.  The sweep fits no Platt probabilities (it reads vote labels only); paa_svc_fit_proba_f64 below fits them.
 * Not served: a model file (the Python layer writes one from paa_svc_fit_proba_f64's outputs).
 *
 * paa_platt_sigmoid_f64 -- probability=True's sigmoid fit alone (svm.cpp: sigmoid_train), one workgroup per PROBLEM:
 *   dec, sign [prob_off[n_problems]]   problem p owns dec[prob_off[p] .. prob_off[p+1]-1], the held-out decision values of one class
 *                            pair, with the signs sign[..] (+1: the pair's first class, -1: the second); 1..8192 values
 * Outputs per problem: A, B of P(first class | dec) = 1 / (1 + exp(A dec + B)); iterations (Newton iterations made); stop
 * (PAA_PLATT_CONVERGED, PAA_PLATT_LINE_SEARCH_FAILED, PAA_PLATT_MAX_ITERATIONS: for the latter two libsvm prints a message and keeps
 * the last A, B; so does this).  sigmoid_train operation for operation in FP64; only the order of its sums over the values
 * differs (fixed by the problem's length alone), so the outputs are bit-identical for a problem alone or in any batch.
 *
 * paa_svc_fit_proba_f64 -- SVC(C, kernel, gamma, probability=True, random_state).fit for every job, in the job form of
 * paa_svc_fit_splits_f64 without test lists, plus seed [n_jobs]: libsvm's random_seed, 0 <= seed < 2^31 (scikit-learn draws it as
 * check_random_state(random_state).randint(np.iinfo('i').max)).  Per pair (a, b), a < b, of the classes present in a job, pair after
 * pair in job order then row-major, with the pair's l rows in PAIR-ROW ORDER (the rows of a in train-list order, then those of b):
 *   - the full fit is one task, as in paa_svc_fit_splits_f64;
 *   - svm_binary_svc_probability's five folds: std::mt19937(seed), restarted for every pair; perm = 0..l-1 shuffled by
 *     j = i + bounded(l - i), swap(perm[i], perm[j]), bounded(range) being Lemire's m = (uint64)r * range with rejection
 *     (if (uint32)m < range, redraw while (uint32)m < (2^32 - range) % range), m >> 32; fold f holds out
 *     perm[f l / 5 .. (f + 1) l / 5 - 1] and trains on the rest, one task whose rows go in permutation order, grouped by class, the
 *     class seen first put first.  A fold whose training part lacks a class makes no task: its held-out values are +1 (only a),
 *     -1 (only b) or 0 (neither);
 *   - all tasks of all jobs are solved side by side, the held-out rows of every fold are scored by the sweep's scoring kernel,
 *     and one launch of the sigmoid kernel fits every pair.
 *   n_pairs, n_rows          must equal the number of pairs the jobs make and the sum of their l
 *   alpha_y [n_rows]         alpha_t y_t of the full fits, pair after pair, each in pair-row order
 *   rho, prob_a, prob_b [n_pairs], n_sv [n_pairs]   of the full fit / of the sigmoid (libsvm's rho, probA, probB)
 *   task_iterations, task_status [n_pairs][6]   slot 0: the full fit, slots 1..5: the folds; status PAA_SMO_CONVERGED /
 *                            PAA_SMO_NOT_CONVERGED, 0 with 0 iterations for a fold that made no task
 *   sig_iterations, sig_stop [n_pairs]   as for paa_platt_sigmoid_f64
 *   cv_dec [n_rows]          (may be NULL) the held-out decision values in pair-row order;  n_launches (may be NULL)
 * Errors are those of paa_svc_fit_splits_f64, raised before the device is touched, plus PAA_ERR_ARG for a seed outside 0..2^31-1.
 * Synchronous, host buffers in and out.  Not served: class weights, shrinking.                                           */
#define PAA_SMO_MAX_ROWS 8192
#define PAA_SMO_MAX_DIMS 256
#define PAA_SMO_CONVERGED 2
#define PAA_SMO_NOT_CONVERGED 3
int paa_smo_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off,
                      const int32_t *task_idx, const int8_t *task_sign, const double *mean, const double *std, const double *C,
                      const double *gamma, int kernel_type, double eps, int max_iter, int iters_per_launch, double *alpha_y,
                      double *rho, int32_t *iterations, double *gap, int32_t *status, int32_t *n_launches);
int paa_svc_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                           const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx,
                           const double *mean, const double *std, const double *C, const double *gamma, int kernel_type,
                           double eps, int max_iter, int iters_per_launch, int32_t *label_out, double *dec_out, int max_pairs,
                           int n_tasks, int32_t *task_iterations, int32_t *task_status, int32_t *task_n_sv, int32_t *n_launches);
#define PAA_PLATT_CONVERGED 0
#define PAA_PLATT_LINE_SEARCH_FAILED 1
#define PAA_PLATT_MAX_ITERATIONS 2
int paa_platt_sigmoid_f64(const double *dec, const int8_t *sign, int n_problems, const int64_t *prob_off, double *A, double *B,
                          int32_t *iterations, int32_t *stop);
int paa_svc_fit_proba_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                          const int64_t *train_off, const int32_t *train_idx, const double *mean, const double *std, const double *C,
                          const double *gamma, int kernel_type, double eps, int max_iter, int iters_per_launch, const int64_t *seed,
                          int n_pairs, int64_t n_rows, double *alpha_y, double *rho, double *prob_a, double *prob_b, int32_t *n_sv,
                          int32_t *task_iterations, int32_t *task_status, int32_t *sig_iterations, int32_t *sig_stop, double *cv_dec,
                          int32_t *n_launches);
/* tests: out6 = threads per workgroup, lane groups, rows per task, test rows per scoring workgroup, default iterations per
 * launch, dims                                                                                                        */
int paa_debug_smo_geometry(int32_t *out6);

/* ---- silence removal of a batch of clips (audioSegmentation.py:672-815), on the device end to end ---------------------------------
 * paa_silence_batch_i16 / _f64 -- the clips lie back to back in `packed` (clip c: samples offsets[c] .. offsets[c + 1] - 1), one
 * sampling rate, window and step (in samples) for all.  Per chunk of whole clips (the device scratch of a chunk stays within 1 GiB,
 * or within chunk_bytes when that is > 0 and smaller; nothing depends on the chunking):
 *   1. the short-term matrices [68][T_c] of the batched plan, which stay in device memory;
 *   2. per clip, tenth = T / 10: quiet_limit = mean of the tenth smallest energies (row 1) + 1e-15, loud_limit = mean of the tenth
 *      largest without one instance of the maximum + 1e-15; the flags energy <= quiet_limit and energy >= loud_limit, their counts;
 *   3. the training rows of every clip -- its quiet frames in frame order, then its loud frames in frame order -- in one matrix
 *      [rows][68], with the clip's scaler: mean and sqrt(var) as NumPy's axis-0 reductions give them, a scale below 10 eps set to 1;
 *   4. per clip SVC(C = 1, linear, probability = True).fit over its standardised rows (quiet: class 0) with libsvm's folds for
 *      seeds[c], as paa_svc_fit_proba_f64 fits one job;
 *   5. the onset probability of every frame (paa_svm_binary_proba_f64's arithmetic with the fit folded into one weight vector),
 *      smoothed by a box of widths[c] frames over the sequence continued by point reflection (untouched for a width < 3);
 *   6. threshold = ((1 - weights[c]) * lowest tenth).mean() + weights[c] * highest tenth.mean() of the smoothed values and the flags
 *      prob > threshold.
 * Errors name the clip: PAA_ERR_ARG for a clip of fewer than 20 frames or fewer than widths[c] (before any device work) and for an
 * empty quiet or loud set, PAA_ERR_UNSUPPORTED for more than 8192 quiet + loud rows (both after step 2 of every chunk and before
 * any fit).
 * Outputs, host arrays.  Per frame, clip after clip: quiet, loud, active (0 / 1), raw (step 5 before smoothing), prob.  Per clip:
 * limits [2], counts [2], mean / scale [68], rho, prob_a, prob_b, threshold, n_sv, iterations / status [6] (slot 0: the full fit,
 * 1..5: the folds), sig_iterations, sig_stop.  Per training row, clip c's rows from row_cap_off[c] (room for min(2 T_c, 8192) rows
 * is enough): src (the row's frame) and alpha_y.  stage_ms [6] (may be null; the stream is drained between the stages when it is
 * not): milliseconds of features, selection, training sets, fits, probability with threshold, copy-back.
 *
 * paa_onset_training_sets_f64 -- steps 2 and 3 for short-term matrices in host memory, [n_dims][frames[c]] blocks back to back
 * (frames[c] >= 20; row 1 is the energy).  src / X [rows][n_dims] receive the rows of all clips back to back (row_capacity: the
 * room in rows; the sum of 2 frames[c] is always enough); a clip without rows has mean 0 and scale 1.
 * paa_onset_activity_f64 -- steps 5 and 6 for such matrices and one linear model per clip: w / mean / scale [n_clips][n_dims],
 * intercept, prob_a, prob_b [n_clips]; dec = <w, (x - mean) / scale> + intercept is scikit-learn's decision_function.            */
int paa_silence_batch_i16(const int16_t *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                          const int32_t *widths, const double *weights, const int64_t *seeds, int64_t chunk_bytes,
                          const int64_t *row_cap_off, uint8_t *quiet, uint8_t *loud, uint8_t *active, double *raw, double *prob,
                          double *limits, int32_t *counts, double *mean, double *scale, int32_t *src, double *alpha_y, double *rho,
                          double *prob_a, double *prob_b, double *threshold, int32_t *n_sv, int32_t *iterations, int32_t *status,
                          int32_t *sig_iterations, int32_t *sig_stop, double *stage_ms);
int paa_silence_batch_f64(const double *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                          const int32_t *widths, const double *weights, const int64_t *seeds, int64_t chunk_bytes,
                          const int64_t *row_cap_off, uint8_t *quiet, uint8_t *loud, uint8_t *active, double *raw, double *prob,
                          double *limits, int32_t *counts, double *mean, double *scale, int32_t *src, double *alpha_y, double *rho,
                          double *prob_a, double *prob_b, double *threshold, int32_t *n_sv, int32_t *iterations, int32_t *status,
                          int32_t *sig_iterations, int32_t *sig_stop, double *stage_ms);
int paa_onset_training_sets_f64(const double *feats, const int32_t *frames, int n_clips, int n_dims, int64_t chunk_bytes,
                                int64_t row_capacity, double *limits, int32_t *counts, uint8_t *quiet, uint8_t *loud, int32_t *src,
                                double *X, double *mean, double *scale);
int paa_onset_activity_f64(const double *feats, const int32_t *frames, int n_clips, int n_dims, const double *w,
                           const double *intercept, const double *prob_a, const double *prob_b, const double *mean,
                           const double *scale, const int32_t *widths, const double *weights, int64_t chunk_bytes, double *raw,
                           double *prob, double *threshold, uint8_t *active);

/* ---- the SVR half of audioTrainTest.evaluate_regression (audioTrainTest.py:774-855 with train_svm_regression :222-226) -----------
 * For "svm" / "svm_rbf" evaluate_regression fits sklearn.svm.SVR(C, kernel) (epsilon 0.1, gamma 'scale') once per split: libsvm's
 * solve_epsilon_svr hands Solver::Solve a dual of 2 n variables over n rows -- variable v stands for row v mod n with the sign +1
 * for v < n and -1 for v >= n, the linear term epsilon - y_t / epsilon + y_t, Q_uv = sign_u sign_v K(row u, row v).  Here a TASK is
 * one such problem over rows of ONE resident sample matrix and its resident targets; one workgroup solves one task with libsvm's
 * Solver without shrinking in FP64 throughout (the selections, TAU, the clip cases and calculate_rho of paa_smo_tasks_f64 over the
 * indices 0 .. 2 n - 1; a kernel row is formed once per ROW and serves both of its variables), and all tasks of a call run side by
 * side, relaunched as paa_smo_tasks_f64 relaunches (iters_per_launch; bit-identical outputs for any value, alone or in any batch).
 *
 * paa_svr_tasks_f64 -- the solver alone:
 *   X [n_samples][n_dims], y [n_samples]   every sample, row-major, and its finite target (1 <= n_dims <= 256, 1 <= n_samples < 2^31)
 *   task_off [n_tasks + 1], task_idx [task_off[n_tasks]]   task t owns the rows task_idx[task_off[t] .. task_off[t+1]-1]; 1..8192 rows
 *   mean, std [n_tasks][n_dims]   task t's standardisation, (x - mean_t) / std_t with an IEEE division on the load path
 *   C, gamma, epsilon [n_tasks]   C > 0; gamma > 0 is read for kernel_type 2 only; epsilon >= 0
 *   kernel_type, eps, max_iter, iters_per_launch   as for paa_smo_tasks_f64
 * Outputs: beta [task_off[n_tasks]] = alpha_t - alpha_{t+n}; per task rho, iterations, gap, status (PAA_SMO_CONVERGED /
 * PAA_SMO_NOT_CONVERGED: outputs are those of the last iterate, finite) and n_sv (rows with beta != 0); train_pred
 * [task_off[n_tasks]], the prediction of every row of the task, G_t - epsilon + y_t - rho from the gradient the solver holds;
 * n_launches may be NULL.  The prediction for a standardised z is sum_t beta_t K(z_t, z) - rho.
 *
 * paa_svr_fit_splits_f64 -- the sweep, in the job form of paa_knn_splits_f64 (train_off / train_idx, test_off / test_idx, mean / std
 * [n_jobs][n_dims]) plus y [n_samples] and C, gamma, epsilon [n_jobs].  Job j is ONE task over its training list in list order; its
 * test rows are scored over the rows with beta != 0 in that order.
 *   pred_out [Q]             the predictions, Q = test_off[n_jobs] rows in job order then test-list order
 *   train_pred_out [train_off[n_jobs]]   (may be NULL) the training predictions of every job, as train_pred above
 *   job_iterations, job_status, job_n_sv [n_jobs]   (each may be NULL);  n_launches (may be NULL)
 * PAA_ERR_ARG, with a message and before the device is touched: a null pointer (other than the optional outputs), offsets that do
 * not begin at 0 or decrease, an index outside 0..n_samples-1, a target that is not finite, n_dims < 1, C <= 0, gamma <= 0 (RBF),
 * epsilon < 0, eps <= 0, kernel_type other than 0 / 2, max_iter < 1, an empty task or training list.  PAA_ERR_UNSUPPORTED, likewise
 * before the device is touched: n_dims > 256 (PAA_SMO_MAX_DIMS), a task of more than 8192 rows (PAA_SMO_MAX_ROWS).  An empty test
 * list is legal.  Synchronous, host buffers in and out.  Not served: nu-SVR, sample weights, a model file.              */
int paa_svr_tasks_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_tasks, const int64_t *task_off,
                      const int32_t *task_idx, const double *mean, const double *std, const double *C, const double *gamma,
                      const double *epsilon, int kernel_type, double eps, int max_iter, int iters_per_launch, double *beta,
                      double *rho, int32_t *iterations, double *gap, int32_t *status, int32_t *n_sv, double *train_pred,
                      int32_t *n_launches);
int paa_svr_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_jobs, const int64_t *train_off,
                           const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx, const double *mean,
                           const double *std, const double *C, const double *gamma, const double *epsilon, int kernel_type,
                           double eps, int max_iter, int iters_per_launch, double *pred_out, double *train_pred_out,
                           int32_t *job_iterations, int32_t *job_status, int32_t *job_n_sv, int32_t *n_launches);

/* ---- the same solver over a RESIDENT kernel matrix ---------------------------------------------------------------------------------
 * paa_svr_tasks_f64 forms two kernel rows per iteration.  Here the n x n matrix of a task is formed once, by the whole device
 * (standardised rows Z, then K in tiles of 32 x 32 values over the upper triangle, mirrored: every value has the bits the solver's own
 * kernel value has), and a second solver reads K(row i, .) and K(row j, .) from it, one thread per row.  Every output is BYTE-EQUAL
 * to the parent's.  The tasks are packed into chunks in task order: the matrix of a task of n rows takes 8 n^2 bytes; a task whose
 * matrix exceeds cache_bytes is solved by the parent's kernel in the same call (cached = 0); any other joins the open chunk when the
 * chunk's matrices and its own fit cache_bytes together, and otherwise opens the next chunk (cached = 1).  Device memory: the largest
 * chunk's matrices plus 8 n pitch bytes of standardised rows per task of it (pitch: n_dims rounded up to 8).
 *
 * paa_svr_tasks_cached_f64, paa_svr_fit_splits_cached_f64 -- the arguments of their parents, then
 *   cache_bytes            the budget in bytes, > 0 (PAA_ERR_ARG otherwise; judged after every argument of the parent)
 *   cached / job_cached    [n_tasks] / [n_jobs] out, not NULL: 1 when the task was solved from its resident matrix
 * Errors are the parents', before the device is touched.
 *
 * paa_svr_gram_f64 -- the matrices alone, for tests: tasks as in paa_svr_tasks_f64 (task_off, task_idx, mean, std, gamma [n_tasks],
 * read for kernel_type 2 only); K_out [sum_t n_t^2]: the full row-major matrix of every task, one after the other; qd_out
 * [task_off[n_tasks]] (may be NULL): the K_tt that the PARENT's solver forms at a task's start (1 for RBF).                          */
int paa_svr_tasks_cached_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_tasks, const int64_t *task_off,
                             const int32_t *task_idx, const double *mean, const double *std, const double *C, const double *gamma,
                             const double *epsilon, int kernel_type, double eps, int max_iter, int iters_per_launch, double *beta,
                             double *rho, int32_t *iterations, double *gap, int32_t *status, int32_t *n_sv, double *train_pred,
                             int32_t *n_launches, int64_t cache_bytes, int32_t *cached);
int paa_svr_fit_splits_cached_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_jobs, const int64_t *train_off,
                                  const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx, const double *mean,
                                  const double *std, const double *C, const double *gamma, const double *epsilon, int kernel_type,
                                  double eps, int max_iter, int iters_per_launch, double *pred_out, double *train_pred_out,
                                  int32_t *job_iterations, int32_t *job_status, int32_t *job_n_sv, int32_t *n_launches,
                                  int64_t cache_bytes, int32_t *job_cached);
int paa_svr_gram_f64(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off, const int32_t *task_idx,
                     const double *mean, const double *std, const double *gamma, int kernel_type, double *K_out, double *qd_out);

/* ---- the C-SVC solver over RESIDENT kernel matrices, shared across a job's tasks --------------------------------------------------
 * paa_smo_tasks_f64 forms two kernel rows per iteration.  The tasks of the classification side share rows: every pair of a job's
 * classes is a task, and with probabilities every pair adds five fold fits over subsets of its rows.  A GROUP is a set of tasks that
 * standardise with the same mean / std and use the same gamma.  Its row list is the distinct sample indices of its tasks in order of
 * first appearance over the tasks in task order; its matrix K [N][N] over that list (8 N^2 bytes) is formed once, by the Gram pass of
 * paa_svr_tasks_cached_f64 (every value has the bits of the solver's own kernel value), and every task of the group reads it through
 * its position list: row t of the task is row pos[t] of the matrix (a sample listed twice maps to one row).  A second solver reads
 * K(row i, .) and K(row j, .) from the matrix, one thread per row; every output is BYTE-EQUAL to the parent's.  The groups are packed
 * into chunks in group order (order of first appearance) by the rule of paa_svr_tasks_cached_f64, applied to the groups' N; the tasks
 * of a group whose matrix alone exceeds cache_bytes are solved by the parent's kernel in the same call.
 *
 * paa_smo_tasks_cached_f64 -- the arguments of paa_smo_tasks_f64, then
 *   group [n_tasks]        tasks with equal ids form a group; NULL: every task is its own group
 *   cache_bytes            the budget in bytes, > 0
 *   cached [n_tasks]       out, not NULL: 1 when the task was solved from its group's resident matrix
 * paa_svc_fit_splits_cached_f64, paa_svc_fit_proba_cached_f64, paa_silence_batch_i16_cached / _f64_cached -- the arguments of their
 * parents, then cache_bytes and job_cached [n_jobs] / clip_cached [n_clips] (out, not NULL).  The group is the JOB (one clip's fit is
 * one job): the full pair fits and all fold fits of a job share one matrix.
 * Errors are the parents', plus PAA_ERR_ARG for cache_bytes <= 0 and for a group whose tasks differ in any byte of their mean, std or
 * gamma (the message names the two tasks); all before the device is touched.
 *
 * paa_debug_smo_cache_layout -- the layout alone, on the host (no device is needed), for tests: the task row lists task_off /
 * task_idx (indices >= 0), group (may be NULL) and cache_bytes as above.  Outputs: n_groups; group_of [n_tasks], the group of every
 * task, numbered in order of first appearance; group_off [n_groups + 1] (room for n_tasks + 1) and group_rows [group_off[n_groups]]
 * (room for task_off[n_tasks]), the groups' row lists; pos [task_off[n_tasks]]; group_chunk [n_groups] (room for n_tasks), the chunk
 * of every group from 0, -1 for a group that is not cached.                                                                        */
int paa_smo_tasks_cached_f64(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off,
                             const int32_t *task_idx, const int8_t *task_sign, const double *mean, const double *std, const double *C,
                             const double *gamma, int kernel_type, double eps, int max_iter, int iters_per_launch, double *alpha_y,
                             double *rho, int32_t *iterations, double *gap, int32_t *status, int32_t *n_launches,
                             const int32_t *group, int64_t cache_bytes, int32_t *cached);
int paa_svc_fit_splits_cached_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                  const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx,
                                  const double *mean, const double *std, const double *C, const double *gamma, int kernel_type,
                                  double eps, int max_iter, int iters_per_launch, int32_t *label_out, double *dec_out, int max_pairs,
                                  int n_tasks, int32_t *task_iterations, int32_t *task_status, int32_t *task_n_sv, int32_t *n_launches,
                                  int64_t cache_bytes, int32_t *job_cached);
int paa_svc_fit_proba_cached_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                 const int64_t *train_off, const int32_t *train_idx, const double *mean, const double *std,
                                 const double *C, const double *gamma, int kernel_type, double eps, int max_iter, int iters_per_launch,
                                 const int64_t *seed, int n_pairs, int64_t n_rows, double *alpha_y, double *rho, double *prob_a,
                                 double *prob_b, int32_t *n_sv, int32_t *task_iterations, int32_t *task_status, int32_t *sig_iterations,
                                 int32_t *sig_stop, double *cv_dec, int32_t *n_launches, int64_t cache_bytes, int32_t *job_cached);
int paa_silence_batch_i16_cached(const int16_t *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                                 const int32_t *widths, const double *weights, const int64_t *seeds, int64_t chunk_bytes,
                                 const int64_t *row_cap_off, uint8_t *quiet, uint8_t *loud, uint8_t *active, double *raw, double *prob,
                                 double *limits, int32_t *counts, double *mean, double *scale, int32_t *src, double *alpha_y,
                                 double *rho, double *prob_a, double *prob_b, double *threshold, int32_t *n_sv, int32_t *iterations,
                                 int32_t *status, int32_t *sig_iterations, int32_t *sig_stop, double *stage_ms, int64_t cache_bytes,
                                 int32_t *clip_cached);
int paa_silence_batch_f64_cached(const double *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                                 const int32_t *widths, const double *weights, const int64_t *seeds, int64_t chunk_bytes,
                                 const int64_t *row_cap_off, uint8_t *quiet, uint8_t *loud, uint8_t *active, double *raw, double *prob,
                                 double *limits, int32_t *counts, double *mean, double *scale, int32_t *src, double *alpha_y,
                                 double *rho, double *prob_a, double *prob_b, double *threshold, int32_t *n_sv, int32_t *iterations,
                                 int32_t *status, int32_t *sig_iterations, int32_t *sig_stop, double *stage_ms, int64_t cache_bytes,
                                 int32_t *clip_cached);
int paa_debug_smo_cache_layout(int n_tasks, const int64_t *task_off, const int32_t *task_idx, const int32_t *group, int64_t cache_bytes,
                               int32_t *n_groups, int32_t *group_of, int64_t *group_off, int32_t *group_rows, int32_t *pos,
                               int32_t *group_chunk);

/* ---- audioTrainTest.regression_wrapper for SVM models (audioTrainTest.py:96-111) ------------------------------------
 * predict() of TRAINED scikit-learn epsilon-SVR models (sklearn.svm.SVR, kernel 'rbf' or 'linear', as
 * train_svm_regression makes them, audioTrainTest.py:222-226) for many feature vectors and many models at once: what
 * file_regression (audioTrainTest.py:1099-1151) asks for once per model_name_* model -- one per target value, each with
 * its own MEANS file -- and evaluate_regression (:774-855) once per test vector of each of its n_exp models per parameter
 * value.  A handle is a BANK of n_models models that share n_dims: model m owns the support vectors sv_offsets[m] ..
 * sv_offsets[m + 1] - 1 of support_vectors [total_sv][n_dims] and dual_coef [total_sv] (scikit-learn's _dual_coef_[0]),
 * rho[m] (= -_intercept_), kernel_type[m] 0 (LINEAR) or 2 (RBF, with gamma[m] = _gamma) and its own standardisation
 * mean[m][n_dims] / std[m][n_dims].  A model with no support vectors is legal (scikit-learn makes one when epsilon exceeds
 * the label spread): it predicts -rho.  1 <= n_models <= 4096, 1 <= n_dims <= 256, offsets from 0 and not decreasing,
 * gamma > 0 for RBF: anything else returns PAA_ERR_ARG, before any device work.  support_vectors / dual_coef may be NULL
 * only when total_sv is 0.
 * feats is feature-major [n_dims][ld], vector v in column v.  out[m][v] = sum_s dual_coef[s] K(sv_s, (x_v - mean_m) / std_m)
 * - rho_m with the support vectors added in the model's order (libsvm's svm_predict_values); a value does not depend on the
 * vector's place in the batch, on n_vec, on ld or on the other models of the bank.  Non-finite inputs are NOT validated
 * (as in paa_svc_*): they propagate by IEEE rules.                                                                   */
int paa_svr_create(int n_models, const int64_t *sv_offsets, const double *support_vectors, const double *dual_coef,
                   const double *rho, const int32_t *kernel_type, const double *gamma, const double *mean, const double *std,
                   int n_dims, void **out_handle);
int paa_svr_destroy(void *handle);
int paa_svr_num_models(const void *handle);
/* host buffers in and out (synchronous): out [n_models][n_vec] */
int paa_svr_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec, double *out);
/* device buffers in and out (the resident mid-term matrix of a plan, paa_plan_mid_execute), asynchronous on the library
 * stream: d_out [n_models][ld_out], ld_out >= n_vec                                                                    */
int paa_svr_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, double *d_out,
                            int64_t ld_out);
/* tests: out4 = windows per workgroup, models per workgroup, support vectors per LDS tile, lanes per window group */
int paa_debug_svr_geometry(int32_t *out4);

/* ---- audioTrainTest.classifier_wrapper for the tree ensembles (audioTrainTest.py:84-93) -------------------------------
 * scikit-learn's RandomForestClassifier / ExtraTreesClassifier (kind PAA_FOREST_AVERAGED) and GradientBoostingClassifier
 * (kind PAA_FOREST_BOOSTED) over many feature vectors at once, as mid_term_file_classification (audioSegmentation.py:583-594)
 * and file_classification (audioTrainTest.py:1091-1095) ask for them once per vector.  The model is scikit-learn's raw
 * per-tree arrays, trees concatenated: tree t owns nodes node_offsets[t] .. node_offsets[t + 1] - 1 and its child indices
 * are local to it (children_left / right = -1 on both sides marks a leaf), feature [nodes] (any value at a leaf),
 * threshold [nodes], missing_go_to_left [nodes] (may be NULL: NaN goes right), value [nodes][n_classes] (averaged: the
 * class fractions of tree_.value) or [nodes] (boosted).  Boosted trees are stage-major: tree s * n_outputs + k is stage s,
 * output k, with n_outputs = 1 for two classes and n_classes otherwise; init [n_outputs] is the constant initial raw score
 * and learning_rate the shrinkage.  Everything is validated before any device work (PAA_ERR_ARG with a message): every
 * child in range and every node reached exactly once from its tree's root, features in 0..n_dims-1, 2 <= n_classes <= 64,
 * 1 <= n_dims <= 256, 1 .. 200 000 trees of at least one node, fewer than 2^31 nodes, whole boosting stages.
 * feats is feature-major [n_dims][ld], vector v in column v; x = (feats - mean) / std in FP64, rounded to float32, and a
 * split goes left when (double)x <= threshold.  label_index [n_vec] receives the class index (-1: a value of x is
 * infinite in float32; -2: a boosted model and a value is NaN -- both are ValueErrors in scikit-learn), proba
 * [n_vec][n_classes] predict_proba, raw [n_vec][n_outputs] (may be NULL) the tree sums in tree order (averaged: before the
 * division by n_trees; boosted: the raw scores before the link).                                                        */
#define PAA_FOREST_AVERAGED 0
#define PAA_FOREST_BOOSTED  1
/* scikit-learn's RandomForestRegressor (audioTrainTest.regression_wrapper, audioTrainTest.py:96-111, as
 * train_random_forest_regression makes it, :229-233): an averaged forest with ONE output.  value [nodes], n_classes must be
 * 1 (for this kind and only for it), learning_rate and init are not read.  proba [n_vec][1] receives the prediction
 * (0.0 + v_0 + v_1 + ... in tree order, divided by n_trees: RandomForestRegressor.predict with n_jobs=None, bit for bit),
 * raw [n_vec][1] the sum before the division, label_index 0 (-1: a value of x is infinite in float32).                */
#define PAA_FOREST_REGRESSOR 2
int paa_forest_create(int kind, int n_trees, const int64_t *node_offsets, const int64_t *children_left,
                      const int64_t *children_right, const int64_t *feature, const double *threshold,
                      const uint8_t *missing_go_to_left, const double *value, int n_classes, int n_dims, double learning_rate,
                      const double *init, void **out_handle);
int paa_forest_destroy(void *handle);
int paa_forest_num_classes(const void *handle);
/* host buffers in and out (synchronous) */
int paa_forest_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec, const double *mean,
                           const double *std, int32_t *label_index, double *proba, double *raw);
/* device buffers in and out (the resident mid-term matrix of a plan, paa_plan_mid_execute), asynchronous on the library
 * stream                                                                                                              */
int paa_forest_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                               const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba,
                               double *d_raw);

/* ---- fitting the tree ensembles: audioTrainTest.train_random_forest / train_extra_trees (audioTrainTest.py:158-178, :202-219) and the
 * forest half of evaluate_classifier (:631-700) -------------------------------------------------------------------------------------
 * A TREE is scikit-learn 1.7.2's DecisionTreeClassifier / ExtraTreeClassifier as its forests fit it: DepthFirstTreeBuilder, Gini,
 * BestSplitter (splitter 0, "randomforest") or RandomSplitter (splitter 1, "extratrees"), max_features = max(1, int(sqrt(n_dims))),
 * min_samples_split 2, min_samples_leaf 1, no depth limit, integer sample weights (a forest's bootstrap counts; 0: the row is out
 * of the bag).  One workgroup builds one tree, all trees of a call side by side, over index lists into ONE resident sample matrix.
 * The builder is restated operation for operation (the float32 input (float)((x - mean) / std), the rand_r xorshift, the
 * Fisher-Yates feature draw with its constant-feature bookkeeping, the 1e-7 candidate rule, the proxy improvement, the thresholds,
 * the leaf rules, the preorder numbering), so every array equals scikit-learn's bit for bit, for a tree alone or at any place of
 * any batch.
 *
 * paa_tree_fit_tasks_f64 -- the trees alone:
 *   X [n_samples][n_dims]    every sample, row-major (1 <= n_dims <= 256, 1 <= n_samples < 2^31)
 *   job_off [n_jobs + 1], job_idx / job_label [job_off[n_jobs]]   job j owns the rows job_idx[job_off[j] .. job_off[j+1]-1] of X with
 *                            the class indices job_label[..] in 0 .. job_k[j] - 1; 1..8192 rows (PAA_TREE_MAX_ROWS), 1..64 classes
 *   mean, std [n_jobs][n_dims]   job j's standardisation
 *   task_job, task_seed [n_tasks]   tree t is fitted on job task_job[t] with the rand_r state task_seed[t] (0 .. 2^32 - 1; scikit-learn
 *                            draws it as RandomState(random_state).randint(0, 2^31 - 1))
 *   task_weight              tree after tree, one weight in 0 .. 8191 per row of the tree's job; one of them must be positive
 *   total_nodes, total_values   the room of the outputs: tree t owns cap_t = 2 (rows of positive weight) - 1 node slots, behind those
 *                            of the trees before it, and cap_t * job_k values likewise
 * Outputs: job_flags [n_jobs] (1: a standardised value is infinite in float32, 2: one is NaN; when any is set NOTHING is fitted and
 * the other outputs are untouched); node_count [n_tasks]; per node slot children_left, children_right (-1: a leaf; tree-local),
 * feature (-2: a leaf), threshold (-2.0), impurity, n_node_samples, weighted_n_node_samples, missing_go_to_left and value
 * [job_k] = the class fractions, as tree_.value holds them.
 *
 * paa_forest_fit_splits_f64 -- the sweep, in the job form of paa_knn_splits_f64 (labels, train_off / train_idx, test_off / test_idx,
 * mean / std [n_jobs][n_dims]) plus n_estimators [n_jobs].  Job j's class indices are re-encoded to the classes PRESENT in its
 * training list, ascending (scikit-learn's np.unique).  Its trees t = sum of n_estimators before j .. take tree_seed [t] and, when
 * tree_weight is not NULL, the weights tree_weight [tree after tree, one per training row of the tree's job] (NULL: every row 1, an
 * ExtraTreesClassifier).  The trees are fitted in chunks of whole jobs within 1 GiB of device scratch, every test row is scored on
 * the device by the kernels of paa_forest_predict_f64 (sum over the trees in tree order, divided by n_estimators, first arg-max);
 * no tree crosses to the host.
 *   label_out [Q]            the class INDEX (a value of `labels`); -1: a test value is infinite in float32
 *   proba [Q][max_classes]   (may be NULL) column c: the job's c-th present class; zeros past a job's classes
 *   job_flags [n_jobs]       as above; when any is set the call stops there and label_out / proba are not valid
 *   n_chunks                 (may be NULL)
 * PAA_ERR_ARG, with a message and before the device is touched: a null pointer (other than the optional ones), offsets that do not
 * begin at 0 or decrease, an index outside 0..n_samples-1, a class index outside its range, an empty job, a weight outside 0..8191, a
 * tree without a positive weight, a seed outside 0..2^32-1, n_estimators < 1, totals that differ from what the tasks make.
 * PAA_ERR_UNSUPPORTED, likewise: n_dims > 256, a job of more than 8192 rows or 64 classes.  Synchronous, host buffers in and out.
 * Not served: other criteria, depth or leaf-size limits, class weights, missing values, gradient boosting (regressors: below). */
#define PAA_TREE_MAX_ROWS 8192
#define PAA_TREE_MAX_WEIGHT 8191
#define PAA_TREE_BEST 0
#define PAA_TREE_RANDOM 1
int paa_tree_fit_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off, const int32_t *job_idx,
                           const int32_t *job_label, const int32_t *job_k, const double *mean, const double *std, int n_tasks,
                           const int32_t *task_job, const int64_t *task_seed, const int32_t *task_weight, int splitter,
                           int64_t total_nodes, int64_t total_values, int32_t *job_flags, int32_t *node_count, int32_t *children_left,
                           int32_t *children_right, int32_t *feature, double *threshold, double *impurity, int32_t *n_node_samples,
                           double *weighted_n_node_samples, uint8_t *missing_go_to_left, double *value);
int paa_forest_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                              const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx,
                              const double *mean, const double *std, const int32_t *n_estimators, int splitter,
                              const int64_t *tree_seed, const int32_t *tree_weight, int32_t *label_out, double *proba, int max_classes,
                              int32_t *job_flags, int32_t *n_chunks);
/* tests: out6 = threads per workgroup, rows per job, classes, dims, the largest weight, MiB of scratch per chunk */
int paa_debug_tree_fit_geometry(int32_t *out6);

/* ---- fitting the forest regressor: audioTrainTest.train_random_forest_regression (audioTrainTest.py:229-233) and the "randomforest"
 * sweep of evaluate_regression (:774-855) ---------------------------------------------------------------------------------------------
 * A regression TREE is scikit-learn 1.7.2's DecisionTreeRegressor as RandomForestRegressor(n_estimators) fits it: the same builder
 * and BestSplitter as above with the squared-error criterion (RegressionCriterion / MSE), max_features = n_dims, one output.  The
 * floating-point sums of a node (sum w y, sum (w y) y, the prefix sums of the candidate scan) are formed in a FIXED order that
 * depends only on the node's rows and the sorted order (kernels_treefit.hpp writes it down; no float atomics), so a tree is
 * bit-identical run to run, alone or anywhere in a batch.  When targets and weights make every such sum exact in FP64 (e.g. targets
 * that are multiples of 1/8 with |y| <= 1024 and a total weight <= 8192) every array equals scikit-learn's bit for bit; otherwise
 * scikit-learn's own summation order (its introsort and in-place partition) is NOT reproduced: the sums may differ in the last
 * places and a tie that rounding breaks may fall the other way -- a valid CART tree, not scikit-learn's bits.
 *
 * paa_tree_fit_reg_tasks_f64 -- the trees alone: the arguments of paa_tree_fit_tasks_f64 with job_target [job_off[n_jobs]] (finite
 * doubles, one per job row) in place of job_label / job_k and without `splitter`; value [total_nodes] holds the node's weighted mean
 * target, so total_values == total_nodes.
 *
 * paa_forest_reg_fit_splits_f64 -- the sweep: the arguments of paa_forest_fit_splits_f64 with targets [n_samples] in place of labels
 * and without `splitter`; tree_weight NULL: every row 1 (no bootstrap).  Same chunking; the trees of a chunk are scored by the
 * kernels of paa_forest_predict_f64 as the averaged forest with one output.
 *   pred [Q]                 the prediction of every test row (sum over the trees in tree order / n_estimators)
 *   train_pred [T]           (may be NULL) the prediction of every job's own training rows, T = train_off[n_jobs]
 *   job_flags [n_jobs]       as above; 1 is also set when a TEST value of the job is infinite in float32; when any is set pred /
 *                            train_pred are not valid
 * Errors as above; PAA_ERR_ARG also for a target (of a job row / a training row) that is not finite.                             */
int paa_tree_fit_reg_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off, const int32_t *job_idx,
                               const double *job_target, const double *mean, const double *std, int n_tasks, const int32_t *task_job,
                               const int64_t *task_seed, const int32_t *task_weight, int64_t total_nodes, int64_t total_values,
                               int32_t *job_flags, int32_t *node_count, int32_t *children_left, int32_t *children_right,
                               int32_t *feature, double *threshold, double *impurity, int32_t *n_node_samples,
                               double *weighted_n_node_samples, uint8_t *missing_go_to_left, double *value);
int paa_forest_reg_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const double *targets, int n_jobs,
                                  const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx,
                                  const double *mean, const double *std, const int32_t *n_estimators, const int64_t *tree_seed,
                                  const int32_t *tree_weight, double *pred, double *train_pred, int32_t *job_flags, int32_t *n_chunks);

/* ---- fitting gradient-boosting classifiers: audioTrainTest.train_gradient_boosting (audioTrainTest.py:181-199) and the
 * "gradientboosting" sweep of evaluate_classifier (:631-700) ---------------------------------------------------------------------
 * The model is scikit-learn 1.7.2's GradientBoostingClassifier(n_estimators) with its defaults: log-loss, subsample 1, the class
 * priors as the initial raw score, and per stage one DecisionTreeRegressor(criterion="friedman_mse", max_depth) per class (one in
 * all for two classes) on the negative gradients, whose leaves take one Newton step (_update_terminal_regions).  A stage's TREE is
 * the regression tree above with FriedmanMSE's proxy and improvement and a depth limit (a node at max_depth is a leaf; the root has
 * depth 0); its sums keep the fixed order, so a model is a function of its job alone: bit-identical run to run, alone or anywhere in
 * a batch, in any chunking.  Where the residual sums are exact in FP64 (stage 0 of balanced jobs with 2, 4 or 8 classes) every tree
 * array and leaf value equals scikit-learn's bit for bit; later stages sum rounded residuals and may differ in the last places.
 *
 * paa_tree_fit_boost_tasks_f64 -- the builder alone: the arguments of paa_tree_fit_reg_tasks_f64 and max_depth (>= 1) before
 * total_nodes; value holds the node means (no leaf step).
 *
 * paa_boost_fit_splits_f64 -- the sweep: X, labels, the train / test lists, mean / std as paa_forest_fit_splits_f64; job j is fitted
 * with n_estimators[j] stages on the classes present among its training rows (at least two, else PAA_ERR_ARG).
 *   tree_seed                the rand_r seed of every tree, job after job, within a job stage-major then by class (one per stage for
 *                            two classes)
 *   init [n_jobs][max_classes]   the initial raw score of every job (its first k_out entries are read; k_out = 1 for two classes)
 *   learning_rate, max_depth scikit-learn's 0.1 and 3
 *   chunk_bytes              <= 0: the 1 GiB rule for the device scratch of one chunk of jobs (a job is never cut); > 0: a smaller
 *                            bound (tests)
 *   label_out [Q]            the class index of every test row (-1: a test value is infinite in float32, -2: it is NaN)
 *   proba [Q][max_classes]   (may be NULL) predict_proba, zeros past a job's classes
 *   train_score [sum of n_estimators]    (may be NULL) per job and stage the mean training loss, scikit-learn's train_score_
 *   train_raw                (may be NULL) per job the raw predictions of its training rows after the last stage, [n][k_out]
 *   train_resid              (may be NULL) per job the negative gradients its LAST stage's trees were fitted to, [n][k_out], as
 *                            boost_gradient_kernel formed them from the raw predictions of the stage before (tests)
 *   total_nodes              0: no trees are returned.  Else the sum over the trees of min(2 n - 1, 2^(max_depth + 1) - 1), and
 *                            node_count .. value receive every tree's scikit-learn arrays in the order of tree_seed, each tree at
 *                            the sum of the sizes before it (value: the Newton value at a leaf, the mean residual elsewhere)
 *   job_flags, n_chunks      as paa_forest_fit_splits_f64
 * Errors as above.                                                                                                                   */
int paa_tree_fit_boost_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off, const int32_t *job_idx,
                                 const double *job_target, const double *mean, const double *std, int n_tasks, const int32_t *task_job,
                                 const int64_t *task_seed, const int32_t *task_weight, int max_depth, int64_t total_nodes,
                                 int64_t total_values, int32_t *job_flags, int32_t *node_count, int32_t *children_left,
                                 int32_t *children_right, int32_t *feature, double *threshold, double *impurity, int32_t *n_node_samples,
                                 double *weighted_n_node_samples, uint8_t *missing_go_to_left, double *value);
int paa_boost_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs, const int64_t *train_off,
                             const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx, const double *mean,
                             const double *std, const int32_t *n_estimators, const int64_t *tree_seed, const double *init,
                             int max_classes, double learning_rate, int max_depth, int64_t chunk_bytes, int32_t *label_out,
                             double *proba, double *train_score, double *train_raw, double *train_resid, int64_t total_nodes,
                             int32_t *node_count,
                             int32_t *children_left, int32_t *children_right, int32_t *feature, double *threshold, double *impurity,
                             int32_t *n_node_samples, double *weighted_n_node_samples, uint8_t *missing_go_to_left, double *value,
                             int32_t *job_flags, int32_t *n_chunks);

/* ---- audioSegmentation.hmm_segmentation / train_hmm_compute_statistics (audioSegmentation.py:287-492) -------------------
 * Gaussian hidden Markov models with one diagonal Gaussian per state, as the reference trains them and hmmlearn's
 * GaussianHMM.predict decodes them.  The model: startprob [K], transmat [K][K], means [K][n_dims], covars [K][n_dims] --
 * covars is what the reference stores in covars_, the per-class STANDARD DEVIATION (audioSegmentation.py:340), and the
 * frame log-likelihood is  B[t][k] = -0.5 (n_dims log 2 pi + sum_d log covars[k][d] + sum_d (x[t][d] - means[k][d])^2 /
 * covars[k][d]).  paa_hmm_create returns PAA_ERR_ARG for K outside 1..32, n_dims outside 1..256, a parameter that is not
 * finite, a covars value <= 0, and a startprob or a transmat row that has a negative entry or does not sum to 1 within
 * 1e-8 (so the 0 / 0 row that the training statistics give for a state that is never left is refused here).
 * feats is feature-major [n_dims][ld], window t in column t, as the mid-term matrix of a plan.  offsets [n_seq + 1] (host
 * memory, also for the device-buffer call) cuts the n_vec windows into independent sequences: offsets[0] = 0,
 * offsets[n_seq] = n_vec, every sequence at least one window (PAA_ERR_ARG otherwise).  Decoding is Viterbi with hmmlearn's
 * semantics: lat[0][j] = log startprob[j] + B[0][j], lat[t][j] = max_i (lat[t-1][i] + log transmat[i][j]) + B[t][j], the
 * last state arg max_j lat[T-1][j], back through arg max_i (lat[t][i] + log transmat[i][s[t+1]]); every arg max is the LOWEST
 * index among equal maxima; log 0 = -inf.  states [n_vec] receives the state of every window, logprob [n_seq] the
 * log-probability of every sequence's best path.  Sequences longer than 256 windows are decoded by blocks of 256 in (max,+)
 * form, which changes the association of the additions: logprob agrees with the serial recursion to rounding, and states
 * agree wherever the serial recursion's decisions are not within rounding of a tie; exact ties between states with
 * identical parameters still resolve to the lowest index.  One decode call per handle at a time (the handle owns the
 * scratch).                                                                                                             */
int paa_hmm_create(const double *startprob, const double *transmat, const double *means, const double *covars, int n_states,
                   int n_dims, void **out_handle);
int paa_hmm_destroy(void *handle);
int paa_hmm_num_states(const void *handle);
/* host buffers in and out (synchronous) */
int paa_hmm_decode_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec, const int64_t *offsets,
                       int64_t n_seq, int32_t *states, double *logprob);
/* device buffers in and out (offsets on the host), asynchronous on the library stream */
int paa_hmm_dev_decode_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                           const int64_t *offsets, int64_t n_seq, int32_t *d_states, double *d_logprob);
/* the frame log-likelihoods B [n_vec][n_states] alone (device buffers, asynchronous) */
int paa_hmm_dev_loglik_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, double *d_loglik);
/* train_hmm_compute_statistics: labels [n_vec] (host) in 0..n_states-1 (PAA_ERR_ARG otherwise); priors [K] = class counts /
 * n_vec, transmat [K][K] = counts of consecutive label pairs divided by their row sums (a state that is never left gives a
 * 0 / 0 = NaN row, as in the reference), means [K][n_dims] and covars [K][n_dims] = np.std (population, two passes) of every
 * feature row over the class's windows.  All four outputs are host arrays; both calls are synchronous.                 */
int paa_hmm_train_stats_f64(const double *feats, int n_dims, int64_t ld, int64_t n_vec, const int32_t *labels, int n_states,
                            double *priors, double *transmat, double *means, double *covars);
int paa_hmm_dev_train_stats_f64(const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, const int32_t *labels,
                                int n_states, double *priors, double *transmat, double *means, double *covars);
/* paa_hmm_dev_decode_f64 with sequences cut every block_rows windows (<= 0: 256); at least the longest sequence: the serial
 * recursion, one wave per sequence                                                                                     */
int paa_debug_hmm_dev_decode_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                 const int64_t *offsets, int64_t n_seq, int32_t *d_states, double *d_logprob,
                                 int64_t block_rows);

/* ---- audioSegmentation.speaker_diarization (audioSegmentation.py:815-1056, lda_dim = 0) -----------------------------------
 * The clustering between the mid-term matrix and the HMM smoothing; every matrix is a device buffer, feature-major
 * [n_dims][ld] (n_dims 1..256), window t in column t; the small results are host arrays and every call is synchronous.
 * standardize: scikit-learn's StandardScaler over the windows (population variance; a constant row gets scale 1); d_z has the
 * layout of d_feats, stats [3][n_dims] = mean, variance, scale.  select_rows: d_out [n_rows][n_vec] = the rows `rows` of d_z.
 * dim_distances: the reference's pdist(X.T) -- Euclidean distances between the n_dims FEATURE ROWS -- over the windows with
 * d_labels[i][t] == c for every sweep entry i < nk and cluster c < ks[i] (d_labels [nk][n_vec] on the device; null: all
 * windows, ks and nk ignored): colsum [nk][kmax][n_dims] the column sums of the distance matrix, pair_mean [nk][kmax] the
 * mean over the n_dims (n_dims - 1) / 2 pairs, kmax = max ks (1 without labels).
 * kmeans: Lloyd's algorithm as scikit-learn 1.7's KMeans(init = centres, n_init = 1) runs it, for all nk cluster counts ks[i]
 * (1..32, at most n_vec) at once: nearest centre in the difference form sum_d (z_d - c_d)^2, lowest index among equal
 * minima; an empty cluster takes the window farthest from its centre; stop when no label changes, or the summed squared
 * centre shift is <= tol, or after max_iter iterations (then one more assignment).  centers [nk][32][n_dims] holds the
 * initial centres on entry and the final ones on return; d_labels [nk][n_vec] (device), n_iter [nk], inertia [nk].  Sums
 * are reduced in a fixed order: two runs give identical bits.
 * sqdist_points: out [n_pts][n_vec] = squared distances of every window to the windows idx[p] (n_pts <= 8): the distance work
 * of k-means++ seeding.  get_points: out [n_pts][n_dims] = the windows idx[p].
 * pair_sums: sums [nk][32][32], sums[i][c][c2] = the sum of |z_a - z_b| over windows a with label c and b with label c2 of
 * sweep entry i, all entries in one pass over the window pairs (difference form, fixed-order reductions).               */
int paa_diar_dev_standardize_f64(const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, double *d_z, double *stats);
int paa_diar_dev_select_rows_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *rows, int n_rows,
                                 double *d_out);
int paa_diar_dev_dim_distances_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *d_labels,
                                   const int32_t *ks, int nk, double *colsum, double *pair_mean);
int paa_diar_dev_sqdist_points_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int64_t *idx, int n_pts,
                                   double *out);
int paa_diar_dev_get_points_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int64_t *idx, int n_pts,
                                double *out);
int paa_diar_dev_kmeans_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *ks, int nk, double *centers,
                            double tol, int max_iter, int32_t *d_labels, int32_t *n_iter, double *inertia);
int paa_diar_dev_pair_sums_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *d_labels,
                               const int32_t *ks, int nk, double *sums);

/* ---- speaker diarization of a batch of clips (audioSegmentation.diarize_features_batch) ---------------------------------------
 * The calls above over MANY clips at once.  The clips lie side by side in ONE device matrix, feature-major [n_dims][ld]
 * (n_dims 1..256): clip i owns the columns cols[i] .. cols[i] + ns[i] - 1 (at most 65535 clips per call).  Clip i's results
 * carry the bits of its own single calls, at any position and beside any other clips.  Both calls are synchronous.
 * prepare: standardize and the all-window dim_distances of every clip; d_z (a buffer of its own, layout of d_feats), stats
 * [n_clips][3][n_dims] = mean, variance, scale, colsum [n_clips][n_dims].  One wait.
 * sweep: k-means for every (clip, k) job and the silhouette's inputs.  Clip i clusters the dims[i] feature rows rows[..] of d_z
 * (the lists of all clips one after the other; the rows are read in place, never compacted) for its nks[i] cluster counts;
 * ks, seeded, first, n_iter and inertia run over the jobs, clip after clip; tols [n_clips] as kmeans' tol.  A job with
 * seeded[j] != 0 is seeded on the device by greedy k-means++ (2 + int(ln k) candidates per step) from numbers the caller drew:
 * first[j] = the first centre's window and, in u (the seeded jobs one after the other), [k - 1][trials] numbers in [0, 1); the
 * potentials, the candidates' sums and the cumulative sum are formed in NumPy's order (pairwise summation per 8192 elements,
 * serial cumsum).  Any other job starts from centers.  centers: [k][dims[i]] per job, one after the other, the given initial
 * centres on entry, the final ones on return.  d_labels (device): [n] per job, one after the other.  a_mean [jobs][32]: the
 * pair_mean of dim_distances per cluster; pair_sums [jobs][32][32] as pair_sums.  stage_ms: null, or [4] = the milliseconds
 * of seeding, k-means and the silhouette inputs (the stream is drained between them) and the Lloyd iterations of the slowest
 * job.  The host waits once per Lloyd iteration of the slowest job and a constant number of times besides.
 * gather: the [n_rows][ns[i]] slabs of a batched plan (clip i at d_slabs + slab_offsets[i]) become the column ranges cols[i] of
 * the matrix d_out [>= n_rows][ld]; queued on the library stream, no wait.                                                */
int paa_diar_batch_gather_f64(const double *d_slabs, int n_rows, const int64_t *slab_offsets, const int64_t *cols,
                              const int64_t *ns, int n_clips, double *d_out, int64_t ld);
int paa_diar_batch_prepare_f64(const double *d_feats, int n_dims, int64_t ld, const int64_t *cols, const int64_t *ns, int n_clips,
                               double *d_z, double *stats, double *colsum);
int paa_diar_batch_sweep_f64(const double *d_z, int n_dims, int64_t ld, int n_clips, const int64_t *cols, const int64_t *ns,
                             const int32_t *dims, const int32_t *rows, const int32_t *nks, const int32_t *ks, const double *tols,
                             int max_iter, const int32_t *seeded, const int64_t *first, const double *u, double *centers,
                             int32_t *d_labels, int32_t *n_iter, double *inertia, double *a_mean, double *pair_sums,
                             double *stage_ms);

/* ---- the LDA step of speaker diarization (audioSegmentation.py:880-934, lda_dim > 0) ------------------------------------------
 * The O(n) parts of scikit-learn's LinearDiscriminantAnalysis (svd solver) on a device matrix, feature-major [n_dims][ld]
 * (n_dims 1..256), window t in column t.  Classes are CONTIGUOUS runs of windows: class c = windows run_offsets[c] ..
 * run_offsets[c + 1] - 1 (host array of n_classes + 1 entries, 0 = first < ... < last = n_vec).  The small results are host
 * arrays and every call is synchronous; the two symmetric eigenproblems between the calls (at most 256 x 256) are the caller's.
 * class_stats: means [n_classes][n_dims] and within_std [n_dims], the population deviation of the windows about their class
 * means over all windows (two passes: means, then deviations), zero replaced by 1 (a NaN stays a NaN).
 * within_gram: gram [n_dims][n_dims] = Xs^T Xs of Xs = sqrt(fac) (x - mean of its class) / within_std, centred and scaled while
 * it is loaded; the upper triangle is computed (FP64 matrix cores) in partials of 1024 windows that are added in window order,
 * the lower triangle is its mirror image.  No floating-point atomics: two runs give identical bits.
 * project: d_y [n_out][ld_y], y[j][t] = sum_d (x[d][t] - xbar[d]) scalings[d][j] (scalings [n_dims][n_out], 1 <= n_out <=
 * n_dims), d ascending.                                                                                                   */
int paa_lda_dev_class_stats_f64(const double *d_x, int n_dims, int64_t ld, int64_t n_vec, const int64_t *run_offsets,
                                int64_t n_classes, double *means, double *within_std);
int paa_lda_dev_within_gram_f64(const double *d_x, int n_dims, int64_t ld, int64_t n_vec, const int64_t *run_offsets,
                                int64_t n_classes, const double *means, const double *within_std, double fac, double *gram);
int paa_lda_dev_project_f64(const double *d_x, int n_dims, int64_t ld, int64_t n_vec, const double *xbar, const double *scalings,
                            int n_out, double *d_y, int64_t ld_y);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------------------------------------- */
#define PAA_COMM_ID_BYTES 128
int paa_comm_unique_id(void *id_out /* PAA_COMM_ID_BYTES, rank 0 only */);
/* one process per GPU: PAA_ERR_COMM when another live rank of the same job (same id) already uses the same physical
 * device on this node (ncclCommInitRank would hang); multi-node jobs and one-visible-device-per-rank launchers are fine */
int paa_comm_init(int world_size, int rank, const void *id);
int paa_comm_destroy(void);
/* gather variable-sized double blocks to rank `root`: counts[world] doubles per rank (host);
 * d_recv (root only) receives them back to back in rank order.  Asynchronous on the stream. */
int paa_comm_gather_f64(const double *d_send, const int64_t *counts, int root, double *d_recv);
/* the same with explicit placement: rank r's block lands at d_recv + displs[r] (in doubles) on the root, so that a job
 * cut into chunks can gather chunk k while chunk k+1 is being computed and still end with one rank-major buffer   */
int paa_comm_gatherv_f64(const double *d_send, const int64_t *counts, const int64_t *displs, int root, double *d_recv);
int paa_comm_barrier(void);

/* ---- introspection for tests (host tables built by the reference's rules) ----------------- */
/* dense mel bank [40][num_fft], dct [13][40]; chroma gather list: returns the number of
 * entries, fills src/weight/slot (capacity entries each) in ascending slot order.            */
int paa_debug_mel_bank(double fs, int num_fft, double *out_dense);
int paa_debug_dct(double *out_13x40);
int paa_debug_chroma(double fs, int num_fft, int capacity, int32_t *src, double *weight, int32_t *slot);
/* the clip constants of a plan (csrc/device_common.hpp: ClipNorm): runs the plan's statistics kernel and clip_params_kernel on
 * d_packed -- also for plans whose feature kernel folds the partials itself -- and waits.  out[0..9] = {samples per statistics
 * chunk, CUs of the device, clips, statistics chunks, norms_inline, sample kind, 0, 0, 0, 0}; then ten doubles per clip: mean, inv,
 * mu, delta_mu, m_int, zb, mu_whole, dc_shift, stat_first, stat_count.  capacity (doubles) >= 10 (clips + 1).  A later
 * paa_plan_execute of the plan computes what it would have computed without this call; needs a device                       */
int paa_debug_plan_clip_norms(paa_plan_t *plan, const void *d_packed, double *out, int64_t capacity);
/* per-phase cycle totals of the fast kernel (diagnostic builds with -DPAA_F800_TIMING; zeros otherwise) */
int paa_debug_wave_trace(uint64_t *out, int max_waves);
int paa_debug_lane_peak(void);     /* most host-buffer calls in flight at once since the last query */
int paa_debug_phase_cycles(uint64_t *out16);
/* radix plan chosen for a window: returns number of passes, fills radices (capacity 32)      */
int paa_debug_fft_plan(int window, int32_t *radices, int32_t *fft_len);
/* HBM-pass path (csrc/kernels_big.hpp: what no other kernel takes) and the frame-list chunks of the workgroup-wide paths, host only:
 * info8 = {complex points Nc, bins Nf, even, passes, scratch bytes per frame, frames per scratch chunk C of a plan whose longest
 * clip has max_frames (>= 1) frames, scratch bytes of that plan, frames per chunk of the workgroup-wide paths' frame list}.  The
 * numbers hold for the window whichever kernel a plan would choose for it                                                        */
int paa_debug_big_plan(int window, int64_t max_frames, int64_t *info8);
/* file name (inside PAA_COMM_MARKER_DIR / TMPDIR) of the one-process-per-GPU marker that `rank` of the job `unique_id`
 * drops for the selected device before RCCL is called (comm_rccl.hpp); needs a device                                */
int paa_debug_comm_marker_name(const void *unique_id, int rank, char *out, int capacity);
/* three-pass register-FFT kernels (csrc/kernels_tri.hpp), host only: shape8 = {R1, R2, R3, packed | group pitch of the second exchange << 8, plane row pitch P, waves per
 * workgroup | H1 << 8 | H2 << 16 (lanes that share a prime butterfly of pass 1 / 2), pass-3 lane jobs, LDS bytes}, offsets6 = SEVEN
 * byte offsets {tw2, p3, g_tw1, g_post, table_bytes, total_bytes, split tables} into the
 * table blob (spectrogram mode: no mel / chroma lists), which is copied to `blob` when that is not NULL.  Returns the blob
 * size, 0 when the window goes to another kernel                                                                     */
int paa_debug_tri_plan(int window, double fs, int32_t *shape8, int32_t *offsets6, unsigned char *blob, int capacity);
/* workgroup-per-frame kernels (csrc/kernels_wg.hpp), host only: info32[48] = {complex points, bins, passes, r0 (0: whole transform in one
 * workgroup's LDS, else r0 sub-transforms whose first pass runs from the samples), elements per (sub-)transform, elements between pad
 * slots, threads, LDS bytes, permutation in LDS, feature kernel stages the row, its LDS bytes, then (radix, span, twiddle stride) per
 * pass}; perm[k] = padded LDS position of output k of the (sub-)transform.  Returns 1, 0 when the window goes to another path        */
int paa_debug_wg_plan(int window, int32_t *info32, uint16_t *perm, int perm_capacity);
/* Real-input split of the 12 x 3675- / 6 x 3675-sample windows (csrc/kernels_wgs.hpp: 44 100 and 22 050 samples -- the 1 s window
 * audioSegmentation.py:1134-1138 passes to feature_extraction at 44.1 / 22.05 kHz), host only: info16 = {r0, points per sub-transform Q,
 * R1, R2, R3 (three register passes), row pitch of the exchange buffer, threads per workgroup, LDS bytes, task types per frame, bins
 * of a spectrum row the feature kernel keeps in LDS (the mel filters' range), its LDS bytes, natural blocks of 64 r0 bins per row (the
 * roll-off is located block by block), threads of the feature kernel}; bin_of[W / 2] (may
 * be null) = the bin that element idx of a UNIT-MAJOR spectrum row holds (the transform kernel stores |X| unit after unit: sub-transform
 * q = 1 .. r0/2 - 1 delivers the bins q + r0 kappa and their mirrors, the last one the bins (r0/2) j).  Returns 1, 0 when the window goes
 * to another kernel                                                                                                                  */
int paa_debug_wgs_plan(int window, int32_t *info16, int32_t *bin_of, int capacity);
/* Host tables of the fused three-pass kernel of the 1 s windows (csrc/kernels_wgr.hpp: 16 000 / 8 000 samples -- the windows
 * audioSegmentation.py:1134-1138 passes to feature_extraction), host only.  mel_job[512][4] = per thread {first bin, index of its weight
 * in the mel table, stride, number of bins}: the thread's share of ONE mel filter (ShortTermFeatures.py:236-254; its bins are first
 * bin + j stride); mel_fil[40][2] = per filter {first thread, threads}; ch_n[12], ch_src[12][64], ch_w[12][64] = the chroma gather lists
 * (:277-321), one entry per lane.  Returns the shape id (1: 20 x 20 x 20, 2: 10 x 20 x 20), 0 when the window goes to another kernel,
 * -1 when a table cannot be held (the plan then keeps csrc/kernels_wg.hpp)                                                         */
int paa_debug_wgr_tables(double fs, int window, int32_t *mel_job, int32_t *mel_fil, int32_t *ch_n, int32_t *ch_src, double *ch_w);
/* ... and its runs of consecutive frames (one workgroup walks runs b, b + grid, ...): per-clip frame counts -> (clip, t0, cnt)
 * triples; *n_runs = their number (runs3 may be NULL to query it)                                                                */
int paa_debug_wgr_runs(const int64_t *frames, int64_t n_clips, int num_cu, int32_t *runs3, int64_t capacity, int64_t *n_runs);
/* Host side of the Bluestein kernel (kernels_blu.hpp: windows whose FFT length has a prime factor above 13; replaces
 * scipy.fftpack.fft at ShortTermFeatures.py:617 for them): info8 = {log2 M, R0, R1, R2, waves per workgroup, LDS bytes,
 * table_bytes, total_bytes}, offsets3 = byte offsets of {conj chirp [W], FFT(b) / M in pass order [M], pass twiddles} in the
 * blob.  Returns the blob size, 0 when the window goes to another kernel (blob may be NULL to query the size). */
int paa_debug_blu_plan(int window, double fs, int32_t *info8, int32_t *offsets3, unsigned char *blob, int capacity);
/* the 64 lane jobs {start, n, woff, ctl} the three-pass kernels cut the sums of n_owners <= 64 owners (40 mel filters / 12 pitch
 * classes) into: owner k has cnt[k] consecutive entries from first[k] (weights from wfirst[k]); a job's ctl = position of the piece
 * in its owner's run of lanes | (lanes k < n_owners: the lane that ends up with owner k's total) << 8 (csrc/kernels_tri.hpp)   */
int paa_debug_lane_jobs(const int32_t *first, const int32_t *wfirst, const int32_t *cnt, int n_owners, int32_t *jobs256);
/* mixed-radix kernel (csrc/kernels_mix.hpp): radix schedule of its in-place DIF transform and the position that holds
 * Z[k] afterwards (perm: fft_len entries); returns the number of passes, 0 when the window goes to another kernel   */
int paa_debug_mix_plan(int window, int32_t *radices, int32_t *fft_len, uint16_t *perm, int perm_capacity,
                       int32_t *waves, int32_t *tw_global);
/* the run-length choice of paa_plan_create for clips of frames[c] frames (host only): runs are multiples of `quantum`
 * frames within [min_run, max_run], cost `halo` extra frames each, a workgroup takes wg_runs of them and num_cu
 * workgroups run at a time.  Returns the cap, the number of runs and the longest run          */
int paa_debug_run_plan(const int64_t *frames, int64_t n_clips, int quantum, int min_run, int max_run, int halo, int wg_runs,
                       int num_cu, int32_t *run_cap, int64_t *n_runs, int32_t *longest);
/* the same for kernels whose runs after a clip's first are `shrink` frames shorter (halo inside the first iteration) */
int paa_debug_run_plan_shrink(const int64_t *frames, int64_t n_clips, int quantum, int min_run, int max_run, int shrink,
                              int wg_runs, int num_cu, int32_t *run_cap, int64_t *n_runs, int32_t *longest);
/* the run lengths a plan that fills LESS than one round of a one-workgroup-per-CU kernel gets instead of equal runs (the hot
 * kernel: num_cu x wg_runs runs whose iteration counts differ by at most one; csrc/lib_plan.hpp: balanced_runs).  Writes them clip
 * after clip to lens[capacity]; returns their number, 0 when the equal runs of `run_cap` stay                              */
int64_t paa_debug_balanced_runs(const int64_t *frames, int64_t n_clips, int run_cap, int quantum, int shrink, int wg_runs,
                                int num_cu, int min_run, int32_t *lens, int64_t capacity);
/* ---- placement of the short runs by XCD (csrc/lib_xcd_order.hpp).  The workgroups of a label (workgroup mod 8) share an XCD;
 * an order is the eight labels, the slowest XCD's first.  PAA_XCD_ORDER=0 in the environment switches probes and orders off.
 * The same cut with the short runs dealt to the labels in `order8` (null: paa_debug_balanced_runs exactly)                  */
int64_t paa_debug_balanced_runs_ordered(const int64_t *frames, int64_t n_clips, int run_cap, int quantum, int shrink, int wg_runs,
                                        int num_cu, int min_run, const int32_t *order8, int32_t *lens, int64_t capacity);
/* puts an order in force on the device until it is cleared (order8 = null: the order the probes had put in force before, or
 * none, is back); probes do not move a forced order.  Plans of paa_plan_create re-cut their tile list at their next execute,
 * plans created later are cut under it                                                                                       */
int paa_debug_xcd_force_order(const int32_t *order8);
/* the calibration of the device: order8 = the order in force (identity when none), tau8 = averaged 100 MHz ticks per iteration of
 * every label (zeros before the first probe), epoch = number of changes of the order in force.  Returns a bit mask: 1 switched
 * on (environment), 2 the device maps labels to XCDs differently (calibration switched itself off), 4 the order is a forced
 * one, 8 an order is in force                                                                                              */
int paa_debug_xcd_state(int32_t *order8, double *tau8, uint64_t *epoch);
/* the run lengths of a balanced plan of paa_plan_create as its next launch would use them (0: not such a plan) and, in info8,
 * {run cap, quantum, shrink, runs per workgroup, shortest run, CUs, 0, 0}: the arguments of paa_debug_balanced_runs for it;
 * epoch = the epoch its list was cut under (0: no order)                                                                      */
int64_t paa_debug_plan_runs(const paa_plan_t *plan, int32_t *lens, int64_t capacity, int32_t *info8, uint64_t *epoch);
/* one execute of such a plan as a probe launch, waited for: record = two words per run (100 MHz counter at the entry of the run's
 * wave; at its exit, with the XCC id the wave ran on in bits 60 .. 63).  The record is checked (a label on more than one XCD
 * switches the calibration off) but not averaged.  Returns the number of runs, 0 when the plan has no probe                   */
int64_t paa_debug_plan_probe(paa_plan_t *plan, const void *d_packed, double *d_out, uint64_t *record, int64_t capacity_runs);

#ifdef __cplusplus
}
#endif
#endif /* PAA_HIP_H */
