/*
 * libdcs -- MI355X (gfx950) separation hot path of MTG/DeepConvSep behind a C ABI.
 *
 * The reference (pure Python 2 + Theano/Lasagne) has no FFI of its own; its
 * integration surfaces are two Python call surfaces:
 *
 *   transformFFT.compute_file / compute_inverse          transform.py:224-274
 *   the separate_*.py train_auto() body                  examples/dsd100/separate_dsd.py:239-313
 *     compute_file -> generate_overlapadd -> predict_function2 ->
 *     overlapadd_multi -> compute_inverse
 *
 * Every entry point below names the reference function whose arithmetic it
 * replaces.  The Python package deepconvsep_amd/ binds these with ctypes and
 * re-creates the reference's function signatures on top.
 *
 * Conventions
 *   - plain C, no exceptions; every function returns 0 (DCS_OK) or a negative
 *     dcs_status; dcs_last_error() gives a thread-local message.
 *   - pointers suffixed _d are DEVICE pointers (HBM), _h are host pointers.
 *     The caller owns every buffer it passes in.
 *   - a dcs_ctx binds one device + one HIP stream; all work of the handles
 *     created from it is enqueued on that stream, asynchronously.  A ctx (and
 *     its plans / models) is not thread-safe; distinct ctx objects are.
 *   - spectrogram matrices are row-major [frames, ld] with ld >= bins; the
 *     "dense" layout of the reference is ld == bins.
 */
#ifndef DCS_H
#define DCS_H

#include <stdint.h>

/* libdcs.so is built with -fvisibility=hidden: the entry points below are the ONLY dynamic symbols it exports. */
#define DCS_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcs_ctx dcs_ctx;
typedef struct dcs_stft dcs_stft;
typedef struct dcs_model dcs_model;
typedef struct dcs_trainer dcs_trainer;

typedef enum {
    DCS_OK = 0,
    DCS_EINVAL = -1,       /* bad argument (shape, size, null pointer)            */
    DCS_EUNSUPPORTED = -2, /* legal in the reference, not built here (see DESIGN) */
    DCS_EHIP = -3,         /* a HIP runtime call failed                            */
    DCS_ENOMEM = -4,       /* device allocation failed                             */
    DCS_ESHAPE = -5        /* parameter count/shape mismatch (set_all_param_values) */
} dcs_status;

/* build_ca variants (examples/<x>/separate_<x>.py) */
enum { DCS_ARCH_DSD = 0, DCS_ARCH_IKALA = 1, DCS_ARCH_BACH10 = 2, DCS_ARCH_BACH10_SI = 3,
       DCS_ARCH_DSD_ILD = 4 /* stereo DSD100 graph of examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:66-115 */,
       DCS_ARCH_IKALA_NOPOOL = 5 /* the iKala TRAINER's graph (examples/ikala/trainCNN.py:87-118): as DCS_ARCH_IKALA without
                                    the (1, 4) max-pool, fc.W has 30 * 21 * 143 = 90 090 rows at 513 bins */,
       DCS_ARCH_BACH10_SI1 = 6 /* the single-branch score-informed graph (examples/bach10_scoreinformed/trainCNNrwc_samp.py:
                                  195-235): 4 input channels, ONE per-source dense layer and pair of InverseLayers, 4 output
                                  channels, 11 arrays -- also what predict_function2 of the 17-array DCS_ARCH_BACH10_SI graph
                                  evaluates (its other three branches never reach the masks) */,
       DCS_ARCH_BACH10_SI_1X1 = 7 /* the deep score-informed graph build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:
                                     66-132): 4 input channels, six strided (1|10 x 5, stride (1, 2)) rectified convolutions with
                                     30 / 50 / 70 / 100 / 200 / 200 filters, a rectified 1x1 convolution of 800 filters sliced into
                                     4 x 200, and per slice the InverseLayers of conv6 .. conv1; 22 arrays (per convolution W, b,
                                     BiasLayer.b, then the final bias of 16).  The live-only layout (1x1 W / b / BiasLayer.b of
                                     200 k rows, final bias of 4 k, k = 1 .. 4) is accepted too; output channels = 4 k.  Needs
                                     time_context >= 19 and F >= 253.  dcs_model_forward / _forward_masked, dcs_model_set_score_semantics
                                     and dcs_separate_scoreinformed take it (tie_mode is ignored: no pooling); the f16 switch, the
                                     one-batch stages and the single-channel / batch / ragged / stereo / spectra paths are
                                     DCS_EUNSUPPORTED.  f32 MFMA throughout (csrc/deep1x1.hip); trained by
                                     csrc/train_deep1x1.hip */ };
/* soft-mask epsilon convention: A = separate_dsd.py:258-266, B = separate_bach10.py:251-259 */
enum { DCS_EPS_A = 0, DCS_EPS_B = 1 };
/* max-pool gradient tie routing: ALL = Theano 0.9 CPU MaxPoolGrad, FIRST = cuDNN */
enum { DCS_TIE_ALL = 0, DCS_TIE_FIRST = 1 };
/* score-informed path, the two places where the separate script and the trainers differ:
 * harmonic masks divided by each instrument's own maximum (script filterSpec, separate_bach10.py:195; dataset.py:781) or, bin by
 * bin, by the sum over the instruments (LargeDatasetMask2.filterSpec, dataset.py:862 -- the class trainCNNrwc.py:657 trains on);
 * soft masks applied to input channel 0 (script, separate_bach10.py:485) or to the sum of the input channels (trainers,
 * trainCNNrwc.py:258-263, trainCNNrwc_samp.py:300-305). */
enum { DCS_SCORE_NORM_MAX = 0, DCS_SCORE_NORM_SUM = 1 };
enum { DCS_MIX_CH0 = 0, DCS_MIX_SUM = 1 };
/* tiler: SCRIPT = separate_dsd.py:114-135 (drops the tail), LIBRARY = util.py:220-248 (zero pads) */
enum { DCS_TILER_SCRIPT = 0, DCS_TILER_LIBRARY = 1 };
/* the update of a trainer (dcs_trainer_set_optimizer): lasagne.updates.adadelta or lasagne.updates.adam */
enum { DCS_OPT_ADADELTA = 0, DCS_OPT_ADAM = 1 };

/* ------------------------------------------------------------------ library / context */
DCS_API int dcs_version(void);
DCS_API const char* dcs_last_error(void);

/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the
 * device's default stream. */
DCS_API int dcs_create(int device, void* hip_stream, dcs_ctx** out);
DCS_API int dcs_destroy(dcs_ctx* ctx);
DCS_API int dcs_synchronize(dcs_ctx* ctx);

/* ------------------------------------------------------------------ framing integers (host) */
/* numberFrames of stft_norm: int(ceil(L/hop) + 2)                      transform.py:309 */
DCS_API int64_t dcs_frame_count(int64_t n_samples, int hop);
/* len(istft_norm(...)) = hop*(T-1) + N - N/2                            transform.py:373,390 */
DCS_API int64_t dcs_inverse_length(int64_t n_frames, int hop, int frame);
/* number of tiles the reference tilers cut from T frames                separate_dsd.py:121-125, util.py:228-232 */
DCS_API int64_t dcs_tile_count(int64_t n_frames, int time_context, int overlap, int tiler);

/* ------------------------------------------------------------------ STFT  (transform.py:224-396) */
/* frame must be a power of two in [64, 8192]; window_h = window(frame) as the reference
 * materialises it in Transforms.__init__ (transform.py:78). */
DCS_API int dcs_stft_plan(dcs_ctx* ctx, int frame, int hop, const double* window_h, dcs_stft** out);
DCS_API int dcs_stft_plan_destroy(dcs_stft* plan);

/* compute_file: mag = |rfft(w * frame)| / sqrt(N), phase = angle(.)     transform.py:243-247
 * audio_d [n_samples]; mag_d / phase_d [rows_out, ld] with rows >= dcs_frame_count() written
 * as zero rows (used by the zero-padding tiler); phase_d may be NULL (phase=False). */
DCS_API int dcs_stft_forward_f32(dcs_stft* plan, const float* audio_d, int64_t n_samples, float* mag_d,
                         float* phase_d, int64_t ld, int64_t rows_out);
DCS_API int dcs_stft_forward_f64(dcs_stft* plan, const double* audio_d, int64_t n_samples, double* mag_d,
                         double* phase_d, int64_t ld, int64_t rows_out);

/* compute_transform (transform.py:80-131; caller examples/dsd100/compute_features.py:83-112): the same transform for every
 * column of audio[t, i] -- n_clips signals of n_samples each, signal c at audio_d + c * clip_stride -- in ONE launch:
 * mag_d / phase_d [n_clips][rows_out, ld], i.e. the reference's mags[i] = compute_file(audio[:, i]) stacked, ready to be
 * written as the .data file.  phase_d may be NULL. */
DCS_API int dcs_stft_forward_f32_clips(dcs_stft* plan, const float* audio_d, int64_t n_samples, int64_t n_clips, int64_t clip_stride,
                               float* mag_d, float* phase_d, int64_t ld, int64_t rows_out);
DCS_API int dcs_stft_forward_f64_clips(dcs_stft* plan, const double* audio_d, int64_t n_samples, int64_t n_clips, int64_t clip_stride,
                               double* mag_d, double* phase_d, int64_t ld, int64_t rows_out);

/* The feature block of one augmented "virtual file", rendered inside the STFT's loader (csrc/fft_render.hip).  Replaces
 * util.circular_shift (util.py:62-81), the time-domain mixing and the chunk slicing of the hiphop feature generators
 * (examples/hiphopss/compute_features.py:55-85, augmentations/compute_features_cs_aug.py:98, :116-147,
 * compute_features_instr_aug.py, compute_features_mix_aug.py:143-231) followed by compute_transform (transform.py:80-131):
 * no rendered signal ever exists.  bank_d [bank_len]: mono source signals back to back.  tracks_h [S][4] int64 = (offset
 * into the bank, length L_s, shift k_s in samples (any sign), output channel c_s in 1 .. S, each once), in the order the
 * reference adds them into the mixture; gains_h [1 + S] = (mixture scale m, g_0 .. g_{S-1}).
 *   r_s[n] = g_s * x_s[n - k_s] if 0 <= n - k_s < L_s else 0,   0 <= n < size
 *   mix[n] = m * (((r_0 + r_1) + r_2) + ...)                     added in list order, no fused multiply-add
 * chunks_h [n_chunks][2] = (a, Lc) with a + Lc <= size; samples outside [a, a + Lc) are zero, as the reference slices the
 * chunk out before it transforms it.  out_d: per chunk one [1 + S][T_c][ld] block, back to back, T_c =
 * dcs_frame_count(Lc, hop) (returned in frames_h [n_chunks]); channel 0 = compute_file(mix chunk), channel c_s =
 * compute_file(r_s chunk); out_rows >= sum (1 + S) T_c.  ONE launch for all chunks.  _f64 takes a float64 bank and equals
 * dcs_stft_forward_f64_clips on the host-rendered chunk bit for bit; _f32 takes a float32 bank.  S 1 .. 8, a track inside
 * the bank, else DCS_EINVAL. */
DCS_API int dcs_stft_forward_render_f64(dcs_stft* plan, const double* bank_d, int64_t bank_len, int S, const int64_t* tracks_h,
                                const double* gains_h, int64_t size, const int64_t* chunks_h, int n_chunks, double* out_d,
                                int64_t ld, int64_t out_rows, int64_t* frames_h);
DCS_API int dcs_stft_forward_render_f32(dcs_stft* plan, const float* bank_d, int64_t bank_len, int S, const int64_t* tracks_h,
                                const double* gains_h, int64_t size, const int64_t* chunks_h, int n_chunks, float* out_d,
                                int64_t ld, int64_t out_rows, int64_t* frames_h);
/* int64 per row of the device table of virtual files dcs_trainer_gather_render reads: (size, a, Lc, T) then S x (offset,
 * L_s, k_s, c_s) */
#define DCS_RENDER_ROW(S) (4 + 4 * (S))

/* The note table of the score renderer (csrc/fft_score_render.hip).  notes_h [sum counts_h][3] int64 = (b: first sample of
 * the note in the rendered track, off: offset of its sample in the bank, len), grouped per track in the order the reference
 * writes them (examples/bach10/compute_features_bach10rwc.py:125-134: each note is ASSIGNED into the track, so a later note
 * overwrites an earlier one where they overlap); counts_h [n_tracks].  packed_h [sum counts_h][4] = (b, off, len, E), E the
 * running maximum of b + len over the track's notes so far.  Host only, no device needed.  b >= 0, len >= 0, [off, off +
 * len) inside the bank, b non-decreasing within a track (what lets the kernel find the covering note of a sample without
 * searching the table), at most 2^31 - 1 notes, else DCS_EINVAL. */
DCS_API int dcs_score_render_pack(const int64_t* notes_h, const int64_t* counts_h, int n_tracks, int64_t bank_len,
                                  int64_t* packed_h);
/* The feature block of one score-rendered virtual file: S tracks assembled note by note from a bank of instrument samples,
 * their mixture, and the transform of each, in ONE launch and without the rendered audio ever existing.  Replaces
 * compute_features_bach10rwc.py:112-139 (the tracks), :139 (the mixture, np.sum over the tracks = the sequential sum in
 * list order) and :141 (compute_transform, transform.py:80-131).  bank_d [bank_len]; notes_h / counts_h [S] as for
 * dcs_score_render_pack, which this call applies.
 *   track_s[n] = bank[off_m + (n - b_m)] for the largest m of track s with b_m <= n < b_m + len_m, else 0   (0 <= n < size)
 *   mix[n]     = ((track_0[n] + track_1[n]) + track_2[n]) + ...
 * out_d [1 + S][T][ld], T = dcs_frame_count(size, hop) (returned in *frames_h if not NULL): channel 0 = compute_file(mix),
 * channel 1 + s = compute_file(track_s); out_rows >= (1 + S) T.  _f64 takes a float64 bank and equals
 * dcs_stft_forward_f64_clips on the host-rendered audio bit for bit; _f32 takes a float32 bank.  S 1 .. 8, ld >= bins, a
 * valid note table, else DCS_EINVAL and nothing is launched. */
DCS_API int dcs_stft_forward_score_render_f64(dcs_stft* plan, const double* bank_d, int64_t bank_len, int S,
                                              const int64_t* notes_h, const int64_t* counts_h, int64_t size, double* out_d,
                                              int64_t ld, int64_t out_rows, int64_t* frames_h);
DCS_API int dcs_stft_forward_score_render_f32(dcs_stft* plan, const float* bank_d, int64_t bank_len, int S,
                                              const int64_t* notes_h, const int64_t* counts_h, int64_t size, float* out_d,
                                              int64_t ld, int64_t out_rows, int64_t* frames_h);
/* int64 per row of the device table of virtual files dcs_trainer_gather_score_render reads: (size, T) then S x (first note,
 * note count) */
#define DCS_SCORE_RENDER_ROW(S) (2 + 2 * (S))

/* compute_inverse for n_src magnitude matrices sharing one phase:       transform.py:271-273, 337-396
 *   X = (mag / pre_div) * sqrt(N) * exp(j*phase) -> irfft -> window -> overlap-add -> / sum(w*w)
 * mag_d [n_src][n_frames, ld] (source stride src_stride elements), phase_d [n_frames, ld],
 * audio_d [n_src][n_out] with n_out <= dcs_inverse_length() (the caller's truncation,
 * separate_dsd.py:305-306).  pre_div is the scale_factor division of separate_dsd.py:304 (1.0 for
 * the plain transform API). */
DCS_API int dcs_stft_inverse_f32(dcs_stft* plan, const float* mag_d, int64_t src_stride, const float* phase_d,
                         int64_t ld, int64_t n_frames, int n_src, float pre_div, float* audio_d,
                         int64_t n_out);
DCS_API int dcs_stft_inverse_f64(dcs_stft* plan, const double* mag_d, int64_t src_stride, const double* phase_d,
                         int64_t ld, int64_t n_frames, int n_src, double pre_div, double* audio_d,
                         int64_t n_out);

/* ------------------------------------------------------------------ tiling (separate_dsd.py:114-169, util.py:220-327) */
/* generate_overlapadd: tiles_d [n, C, tc, F] = scale * mag_d[C][T, ld] windows; n = dcs_tile_count().
 * (the reference multiplies by scale_factor before tiling, separate_dsd.py:290) */
DCS_API int dcs_tile(dcs_ctx* ctx, const float* mag_d, int64_t ch_stride, int64_t ld, int C, int64_t n_frames, int F,
             int time_context, int overlap, int tiler, float scale, float* tiles_d, int64_t n_tiles);

/* overlapadd_multi / overlapadd: cross-fade stitch of out_d [S, n, tc, F] into
 * sep_d [S][n*(tc-ov)+tc, ld] (source stride sep_stride).  rise_h = np.linspace(0,1,overlap) as
 * float64 (util.py:306); the fall ramp is its reverse (util.py:307). */
DCS_API int dcs_overlap_add(dcs_ctx* ctx, const float* out_d, int64_t n_tiles, int S, int time_context, int overlap,
                    int F, const double* rise_h, float* sep_d, int64_t sep_stride, int64_t ld);

/* ------------------------------------------------------------------ network (build_ca + mask) */
/* params_d: device float32 arrays in lasagne.layers.get_all_params order (= the .pkl order),
 * shapes: nparams x 4 int64 (unused trailing dims = 1).  Fails with DCS_ESHAPE exactly where
 * lasagne.layers.set_all_param_values would raise (separate_dsd.py:250). */
DCS_API int dcs_model_create(dcs_ctx* ctx, int arch, int in_channels, int time_context, int F,
                     const float* const* params_d, const int64_t* shapes, int nparams, dcs_model** out);
DCS_API int dcs_model_destroy(dcs_model* m);
DCS_API int dcs_model_num_sources(const dcs_model* m);
/* f16 = 1: conv2 and its transpose of the ikala / bach10 / score-informed graphs run with f16 inputs and
 * f32 accumulation on the matrix cores (BASELINE config 3, "fp16 MFMA conv path"); 0 (default): f32-class arithmetic
 * everywhere (f32 MFMA, or the bf16 pipe with operands split exactly into three bf16 terms).  With the switch on, the
 * single-channel bach10 graph runs both InverseLayers in one kernel (colconv_wreg.hip): conv2^T in f16 and -- the default since
 * round 4 -- conv1^T in f16 as well: the activations between the two InverseLayers are rounded to f16 and meet an f16 conv1
 * filter in one MFMA per tile (f32 accumulation).  Results stay within the f16 path's stated tolerance (2e-3 of the network
 * output, tests/test_gpu_configs.py), not within 1e-4.  Since round 6 the DENSE layers of that graph follow the switch as well
 * when a pass has 128 .. 176 tiles (the window of the all-rows kernels): the bottleneck layer and the per-source layers multiply
 * f16 weights (one plane, 2 bytes per weight -- SURVEY 8d prices this config as HBM-on-weights at fp16), conv1 hands its map to
 * conv2 as f16 (the same values conv2 rounded to before, now rounded once by the producer), conv2 hands its map to
 * the bottleneck layer as f16, and the per-source layers write their output once as f16 in the layout the fused decoder reads
 * (gemm_f16.hip); the measured error of the network output is unchanged (3e-5: the f16 convolutions dominate).  The ikala
 * graph (10 x 20 filters) takes the same slab kernel in either precision (one f16 plane instead of three bf16 planes). */
DCS_API int dcs_model_set_conv_precision(dcs_model* m, int f16);
/* Score-informed graphs (DCS_ARCH_BACH10_SI / _SI1 / _SI_1X1): which of the reference's two semantics dcs_separate_scoreinformed and
 * dcs_model_forward_masked follow (the enums above).  Default = the separate script's: DCS_SCORE_NORM_MAX, DCS_MIX_CH0.
 * A model trained by trainCNNrwc.py saw sum-normalised inputs and a channel-sum mixture: (DCS_SCORE_NORM_SUM, DCS_MIX_SUM).
 * DCS_MIX_SUM adds the C input channels left to right in float32.  DCS_EUNSUPPORTED for single-channel graphs. */
DCS_API int dcs_model_set_score_semantics(dcs_model* m, int normalise, int mixture);
/* Which stages of dcs_separate run on the one-batch ("latency") kernels of csrc/dsd_lat.hip -- the shape of the
 * reference's own call, predict_function2 on ONE batch of 32 tiles (separate_dsd.py:296-298), where a kernel's duration
 * is its chain of dependent memory latencies.  stages = -1 (default): automatic, all of them for one clip of at most
 * 1024 frames; 0: the throughput kernels; else a bit set: 1 STFT, 2 conv1, 4 conv2, 8 bottleneck,
 * 16 per-source dense, 32 transposed conv2, 64 final (transposed conv1 + mask + cross-fade), 128 iSTFT.  Both families
 * read and write the same buffers, so any mix is valid (tests compare each stage against the other family).  DSD graph
 * only (DCS_EUNSUPPORTED otherwise). */
DCS_API int dcs_model_set_latency_stages(dcs_model* m, int stages);
/* Testing aids (host only, no GPU): the weight re-layouts of the one-batch kernels.  dcs_lat_pack_b_host: B[K][ldb]
 * (k-major) -> [slice][column block][j][lane][4], the order in which lane (fi = lane & 15, kq = lane >> 4) of wave
 * `slice` feeds v_mfma_f32_16x16x4_f32: element e of piece j is B[slice * slice_len + 16 j + 4 kq + e][16 cb + fi].
 * dcs_lat_pack_deconv2_host: Bw2s[ci][16 taps][52] -> [ci][j][lane][4] with column fi = tap.  Both return the number of
 * floats of the packed array (and fill `out` when out_len is large enough) or a negative status. */
DCS_API int64_t dcs_lat_pack_b_host(const float* B, int ldb, int K, int n_cb, int slice_len, int n_slices, float* out, int64_t out_len);
DCS_API int64_t dcs_lat_pack_deconv2_host(const float* Bw2s, int n_ci8, float* out, int64_t out_len);

/* predict_function2 (separate_dsd.py:273,298): tiles_d [n, C, tc, F] -> out_d [S, n, tc, F]
 * = soft-masked magnitudes of the S sources. */
DCS_API int dcs_model_forward_masked(dcs_model* m, const float* tiles_d, int64_t n_tiles, int eps_mode, int tie_mode,
                             float* out_d);
/* lasagne.layers.get_output(network2): p_d [n, channels_out, tc, F] before masking (testing aid) */
DCS_API int dcs_model_forward(dcs_model* m, const float* tiles_d, int64_t n_tiles, int tie_mode, float* p_d);
/* The same for the stereo (ILD) graph (DCS_ARCH_DSD_ILD, else DCS_EINVAL), which dcs_model_forward refuses: tiles in the ROW
 * layout of dcs_separate_stereo, the C = 2 channels of a frame side by side.  tiles_d [n_tiles][tc][C][ld], ld = F rounded up
 * to 4, 16-byte aligned, columns F .. ld-1 ZERO on entry; every tile is encoded from its own tc rows.  p_d [S = 4][n_tiles tc]
 * [C ld]: the rectified network output (output BiasLayer and rectifier applied, no mask) -- source s, input channel c is the
 * reference's output channel s C + c (trainCNN_ILD_DSD100.py:106-111); columns F .. ld-1 of each channel are unspecified.
 * DCS_EINVAL for a NULL pointer or a negative count; n_tiles == 0 does nothing.  What a stereo stream (below) runs between
 * its push and its pull. */
DCS_API int dcs_model_forward_stereo(dcs_model* m, const float* tiles_d, int64_t n_tiles, float* p_d);
DCS_API int dcs_model_out_channels(const dcs_model* m);
/* Which kernel the fused path (dcs_separate*) runs for the decoder's last stage (transposed conv1 + bias + rectify + mask
 * + cross-fade) on n_clips clips of n_frames frames each: 0 = f32 MFMA, 64-bin workgroups (small launches); 1 = f32
 * MFMA, 128-bin workgroups; 2 = bf16 MFMA on operands split exactly into three bf16 terms (f32-class results, the
 * default for launches that fill the chip; DSD / hiphop graph); 3 = the one-batch kernel of csrc/dsd_lat.hip (one clip of
 * at most 1024 frames, see dcs_model_set_latency_stages; the same bf16x3 arithmetic, 16 x 64 workgroups);
 * negative: not a fused-kernel graph.  bench.py prices its roofline block with this. */
DCS_API int dcs_model_final_kernel(const dcs_model* m, int64_t n_frames, int64_t n_clips, int eps_mode);

/* ------------------------------------------------------------------ fused file-level path */
/* The separation block of train_auto (separate_dsd.py:289-306) for one mono signal already in
 * HBM:  STFT -> x scale -> tiles -> network -> mask -> cross-fade overlap-add -> / scale ->
 * iSTFT -> truncate to n_samples.  pcm_d [S, n_samples] float32.  n_tiles_out / n_frames_out
 * (host, optional) receive the tile and frame counts.  Returns DCS_EINVAL when the tiler yields
 * zero tiles (the reference raises in overlapadd_multi in that case). */
DCS_API int dcs_separate(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int overlap, int tiler,
                 float scale, int eps_mode, int tie_mode, float* pcm_d, int64_t* n_tiles_out,
                 int64_t* n_frames_out);

/* The separation block of the score-informed script (examples/bach10_scoreinformed/separate_bach10.py:497-571) in one
 * call: STFT -> x scale -> filterSpec masks of the note table (notes_h exactly as for dcs_score_masks, frame window
 * (0, n_frames)) -> ninst-channel tiles of the library tiler -> network -> masks (applied to input channel 0, or to the channel
 * sum after dcs_model_set_score_semantics; the same call selects the sum-normalised harmonic masks) -> cross-fade
 * -> / scale -> iSTFT.  The model must have ninst input channels.  pcm_d [S, n_samples] float32.  All tiles go through the
 * network in one pass (the script's batch loop gives the same values tile by tile).  Asynchronous (the note rectangles are
 * staged through the context's pinned upload ring; notes_h may be reused when the call returns). */
DCS_API int dcs_separate_scoreinformed(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, const double* notes_h,
                               int ninst, int n_notes, int width, int overlap, float scale, int eps_mode, int tie_mode,
                               float* pcm_d, int64_t* n_tiles_out, int64_t* n_frames_out);

/* The same pipeline for n_clips mono signals of EQUAL length in one set of launches (the batch-of-files
 * driver of SURVEY 8f.1 / separate_multiple.ipynb; equal-length segments of one long file): clip c starts at
 * audio_d + c * clip_stride (clip_stride >= n_samples), pcm_d [n_clips][S][n_samples].  Every clip is processed
 * exactly as dcs_separate would process it alone (same tiles, same cross-fade) -- the clips only share kernel
 * launches; outputs agree with the single-clip call to fp32 rounding (the FFT / GEMM kernel variants are
 * chosen by the total amount of work).  The ikala / bach10 graphs stack the tiles of all clips into one pass of the
 * network (their dense-layer weights are then read once per group).  n_tiles_out / n_frames_out are per clip. */
DCS_API int dcs_separate_batch(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int64_t n_clips,
                       int64_t clip_stride, int overlap, int tiler, float scale, int eps_mode, int tie_mode,
                       float* pcm_d, int64_t* n_tiles_out, int64_t* n_frames_out);

/* The same for clips of DIFFERENT lengths (a directory of songs, separate_multiple.ipynb): clip c has
 * n_samples_h[c] samples (host array) starting at audio_d + c * clip_stride, and its S signals are written to
 * pcm_d + (c * S + s) * pcm_stride (pcm_stride >= the longest clip; samples past a clip's own length are not
 * written).  Strides and grids are sized by the longest clip; the STFT, the cross-fade fold and the iSTFT read
 * every clip's own sample / frame / tile counts from a small device table, so each clip gets exactly the frames,
 * the tiles and the cross-fade dcs_separate gives it alone (shorter clips cost the launch the work of the longest).
 * Every single-channel graph: DSD / hiphop through the fused path; ikala / bach10 with one STFT / iSTFT launch over all
 * clips and one pass of all their tiles through the network (a clip's tiles sit behind those of the clips before it).
 * Needs the wave STFT kernels (frameSize 1024 / 2048 / 4096 with hop | frameSize, DCS_EUNSUPPORTED otherwise).
 * n_tiles_out / n_frames_out: [n_clips] or NULL.  Equal lengths with pcm_stride == length take the
 * dcs_separate_batch path.  Asynchronous like every other call: the clip table goes out through a pinned staging ring owned
 * by the model (n_samples_h may be reused as soon as the call returns). */
DCS_API int dcs_separate_ragged(dcs_model* m, dcs_stft* plan, const float* audio_d, const int64_t* n_samples_h,
                        int64_t n_clips, int64_t clip_stride, int overlap, int tiler, float scale, int eps_mode,
                        int tie_mode, float* pcm_d, int64_t pcm_stride, int64_t* n_tiles_out, int64_t* n_frames_out);

/* Stereo separation, the "Separating" block of examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:291-325, for a
 * DCS_ARCH_DSD_ILD model: audio_d holds the two channels (channel c at audio_d + c * channel_stride), one STFT per
 * channel, 2-channel tiles (pass DCS_TILER_LIBRARY: the trainer calls util.generate_overlapadd), one network pass,
 * per input channel the mask of :176-180 (p / (sum over sources + 1e-12 r), source = mask * input + 1e-12 r, r = 0.1
 * standing in for the trainer's N(0, 0.1) draw), cross-fade, and the iSTFT with that channel's phase.
 * pcm_d [2][S][n_samples]; sep_d (optional) [2][S][n_frames, ld_out] scaled magnitudes.  Either may be NULL. */
DCS_API int dcs_separate_stereo(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int64_t channel_stride,
                        int overlap, int tiler, float scale, float* pcm_d, float* sep_d, int64_t ld_out,
                        int64_t* n_tiles_out, int64_t* n_frames_out);

/* Same pipeline stopped before the iSTFT: sep_d [S][n_frames, ld_out] (scaled magnitudes, what the
 * reference calls mm[i,:len(ph)]) and phase_d [n_frames, ld_out]; either may be NULL. */
DCS_API int dcs_separate_spectra(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int overlap,
                         int tiler, float scale, int eps_mode, int tie_mode, float* sep_d, float* mag_d,
                         float* phase_d, int64_t ld_out);

/* The wav sample format of every script: out_d[i] = (int16)(pcm_d[i] * 32767), truncation toward zero, no
 * clipping (separate_dsd.py:307-309); the product is formed in double like the scripts' float64 `audio_out * maxn`, so the
 * values are those of `(pcm.astype(float64) * 32767).astype('int16')` bit for bit.  Halves the bytes of the multi-GPU PCM
 * gather and of the batch driver's device-to-host copy. */
DCS_API int dcs_pcm_to_int16(dcs_ctx* ctx, const float* pcm_d, int64_t n, int16_t* out_d);

/* The other end of a wav file: int16 frames as scipy.io.wavfile.read returns them ([n_frames][channels], interleaved) -> the
 * mono float32 signal the scripts separate: sample.astype('float') / 32767 (separate_dsd.py:275-282, float64), then
 * mode 0: (L + R) / 2 for two or more channels, the channel itself for mono (separate_dsd.py:285-287, separate_bach10.py);
 * mode 1: L + R (separate_ikala.py:229; a mono file is DCS_EINVAL with NumPy's IndexError text), computed in double and
 * rounded to float32 once -- the value the host path `to_device(to_mono(read_wav(f)))` uploads, bit for bit, for half (stereo)
 * or a quarter (mono) of its PCIe bytes and none of its host arithmetic.  n_clips stacked clips: clip c at
 * pcm16_d + c * in_stride (int16 elements, >= n_frames * channels), out_d + c * out_stride. */
DCS_API int dcs_pcm16_to_float(dcs_ctx* ctx, const int16_t* pcm16_d, int64_t n_frames, int channels, int mode, int64_t n_clips,
                       int64_t in_stride, float* out_d, int64_t out_stride);

/* ---- wav files of the batch-of-files driver (host side, no device work) ----------------------------------------------
 * What scipy.io.wavfile.read / .write do in every script (separate_dsd.py:275-282, :307-309) for 16-bit PCM files, by a pool of
 * I/O threads and without the float detour: int16 frames go from the file into the caller's (pinned) staging memory and from
 * it into a file behind the 44-byte header scipy.io.wavfile.write produces -- the division by 32767, the mix-down and the int16
 * conversion are dcs_pcm16_to_float / dcs_pcm_to_int16 on the device.  A batch of reads or writes is one call that returns at
 * once; the caller collects it with dcs_wav_batch_wait.  Thread-safe; the threads never call back into the caller. */
typedef struct dcs_wav_pool dcs_wav_pool;
typedef struct dcs_wav_batch dcs_wav_batch;
DCS_API int dcs_wav_pool_create(int n_threads, dcs_wav_pool** out);
/* Completes every enqueued batch first.  Batches that were not waited for stay valid for dcs_wav_batch_wait. */
DCS_API void dcs_wav_pool_destroy(dcs_wav_pool* pool);
/* Enqueue n reads.  File i: its frames go to dst_h[i] (capacity cap[i] bytes); after the wait status[i] is 0 (rate[i],
 * n_frames[i], channels[i] are set, the frames lie at dst_h[i] as [n_frames][channels] int16), 1 (not plain 16-bit PCM, e.g.
 * float / 24-bit samples, a damaged header, or larger than cap[i]: take the scripts' float path for this file) or -errno (the
 * file could not be opened or read).  The paths are copied; every other array must stay valid until the wait. */
DCS_API int dcs_wav_read_pcm16_async(dcs_wav_pool* pool, int n, const char* const* paths, void* const* dst_h, const int64_t* cap,
                                     int32_t* rate, int64_t* n_frames, int32_t* channels, int32_t* status, dcs_wav_batch** out);
/* Enqueue n writes.  File i = the 44 header bytes of scipy.io.wavfile.write(path, rate[i], int16 [n_frames[i]] or
 * [n_frames[i], channels[i]]) followed by the frames at data_h[i], one writev; missing parent directories are created.
 * status[i] after the wait: 0 or -errno.  DCS_EINVAL for a file that would not fit a wav header (>= 4 GiB). */
DCS_API int dcs_wav_write_pcm16_async(dcs_wav_pool* pool, int n, const char* const* paths, const int16_t* const* data_h,
                                      const int64_t* n_frames, const int32_t* channels, const int32_t* rate, int32_t* status,
                                      dcs_wav_batch** out);
/* 1 when every file of the batch has been handled (the batch stays valid), 0 otherwise. */
DCS_API int dcs_wav_batch_done(dcs_wav_batch* batch);
/* Blocks until the batch is complete and releases it. */
DCS_API int dcs_wav_batch_wait(dcs_wav_batch* batch);

/* The one exchange of the multi-GPU path (tiles / clips are sharded over one process per GPU and nothing else is shared;
 * SURVEY 8b `dcs_gather(h, ncclComm_t, shard, count, full, root)`, counted in BYTES here so that the scripts' int16 PCM of
 * dcs_pcm_to_int16 travels as it is).  nccl_comm is the caller's ncclComm_t (RCCL: ncclCommInitRank, one rank per GPU);
 * librccl is dlopen'ed on first use -- libdcs has no link-time dependency on it (DCS_EUNSUPPORTED if it cannot be loaded).
 * root < 0: all-gather, every rank's full_d [n_ranks][bytes] in rank order.  root >= 0: only that rank receives (grouped
 * ncclSend / ncclRecv: what a single writer process needs, 1 / n_ranks of the all-gather's traffic per link); full_d may be
 * NULL elsewhere.  Enqueued on the ctx stream like every other call; shard_d may be the rank's own slot of full_d. */
DCS_API int dcs_gather(dcs_ctx* ctx, void* nccl_comm, const void* shard_d, int64_t bytes, void* full_d, int root);

/* ------------------------------------------------------------------ score-informed front-end */
/* filterSpec (examples/bach10_scoreinformed/separate_bach10.py:172-200) and the network input of :520-527.
 * notes_h: HOST table [ninst][n_notes][width] of doubles exactly as expandMidi returns it (util.py:424-512),
 * width = 2*nharmonics+3: begin frame, end frame, midi number, then (first bin, one-past-last bin) pairs, zeros
 * unused.  start/stop: filterSpec's frame window (0, nframes in the script).  Per instrument j the mask is 1 on
 * the note rectangles and 1e-18 elsewhere, divided by its maximum (so an instrument without notes gets an all-ones
 * mask, as in the reference).  out_d [ninst][n_frames][F] = mask_j * mag_d (mag_d [n_frames, ld], already scaled by
 * the caller like :503); mask_d [n_frames][ninst*F] = filterSpec's return value.  Either output may be NULL.
 * A bin range outside [0, F) is DCS_ESHAPE (NumPy raises IndexError there).  Asynchronous: the note rectangles go out through
 * a pinned staging ring owned by the context. */
DCS_API int dcs_score_masks(dcs_ctx* ctx, const float* mag_d, int64_t ld, int64_t n_frames, int F, const double* notes_h,
                    int ninst, int n_notes, int width, int64_t start, int64_t stop, float* out_d, float* mask_d);

/* The same with the normalisation of the masks chosen by the caller: DCS_SCORE_NORM_MAX = dcs_score_masks; DCS_SCORE_NORM_SUM =
 * LargeDatasetMask2.filterSpec (dataset.py:839-879): mask_j = filtered_j / sum_i filtered_i, float32, instruments added in order
 * -- a bin nobody plays is 1e-18 / (4 x 1e-18 added in turn) = 0.25 for four instruments, a bin k instruments play is 1 / k for
 * them and 1e-18 / k for the others.  At most 32 instruments. */
DCS_API int dcs_score_masks_norm(dcs_ctx* ctx, const float* mag_d, int64_t ld, int64_t n_frames, int F, const double* notes_h,
                         int ninst, int n_notes, int width, int64_t start, int64_t stop, int normalise, float* out_d,
                         float* mask_d);

/* ------------------------------------------------------------------ BSS Eval v3 energies (deepconvsep_amd/evaluation.py) */
/* The separation-quality step the reference runs in MATLAB after separating: bss_eval_sources
 * (evaluation/bss_eval/bss_eval_sources.m; evaluation/evaluate_SS_iKala.m, evaluation/Bach10_eval_only.m), bss_eval_images
 * (evaluation/bss_eval/bss_eval_images.m) and its framewise driver bss_eval (evaluation/DSD100_eval_only.m), restated as the
 * five energies every criterion follows from (DESIGN.md "BSS Eval").  float64 throughout; deterministic (no atomics).
 *
 * Layout: ref_d [nsrc_ref * nchan][nsampl] and est_d [nsrc_est * nchan][nsampl], row k = source * nchan + channel, float64
 * device arrays.  Window w covers samples [w * hop, w * hop + win) and is evaluated as an isolated signal (zero outside);
 * (nwin - 1) * hop + win <= nsampl.  flen: distortion filter length, a multiple of 16 in [16, 512] (512 in the reference).
 * At most 16 reference and 16 estimate channels (DCS_EUNSUPPORTED beyond).
 *
 * out_d [nwin][nsrc_est][nsrc_ref][nchan][5] with all_pairs != 0, [nwin][nsrc][nchan][5] (jest == jtrue) with all_pairs == 0
 * (then nsrc_est == nsrc_ref).  For estimate channel e = est(jest, i) and s = ref(jtrue, i), the five float64 are
 *   ||e||^2, ||s||^2, <e, s>, ||P_jtrue e||^2, ||e - P_all e||^2
 * where P_j / P_all project orthogonally, in the zero-padded domain of length win + flen - 1, onto the span of r_k(t - a),
 * a in [0, flen), k over the channels of source j / over all channels.  A pivot <= N * eps * max(diag G) of the Gram matrix
 * (N its order) drops its basis vector, so a silent or dependent reference channel leaves the span without harm.
 * Window groups bound the scratch to ~3 GB for any length.  Enqueued on the ctx stream. */
DCS_API int dcs_bss_energies(dcs_ctx* ctx, const double* ref_d, const double* est_d, int nsrc_ref, int nsrc_est, int nchan,
                             int64_t nsampl, int64_t win, int64_t hop, int64_t nwin, int flen, int all_pairs, double* out_d);

/* Stage (a) of dcs_bss_energies alone, for one whole signal: out_d[k][n][d + flen - 1] = sum_t r_k(t + d) z_n(t),
 * d in [-(flen - 1), flen - 1], k < n_ref, z = the n_ref rows of ref_d then the n_est rows of est_d ([n][n_samples] each),
 * signals zero outside [0, n_samples).  The Gram matrix of the delayed references is G[(k1,a),(k2,b)] = c_{k1,k2}(b - a)
 * (the correlations bss_eval_sources.m / bss_eval_images.m take with fftfilt).  Enqueued on the ctx stream. */
DCS_API int dcs_bss_lagcorr(dcs_ctx* ctx, const double* ref_d, const double* est_d, int n_ref, int n_est, int64_t n_samples,
                            int flen, double* out_d);

/* ------------------------------------------------------------------ score-to-audio alignment (csrc/align.hip) */
/* What puts a score at nominal tempo onto the recording before dcs_score_masks paints it (the reference never needed it:
 * Bach10 ships hand-aligned scores).  Chroma of a magnitude spectrogram: mag_d [n_frames, ld] float32, cls_h [F] on the HOST,
 * the pitch class 0 .. 11 of every bin or -1 for a bin that is not used (uploaded through the context's ring, no
 * synchronisation); chroma_d [n_frames][12]:
 *   c_k = sum_{f: cls[f] = k} mag[t, f],  n = sqrt(sum_k c_k^2),  row = c / n if n > floor, else twelve times 1 / sqrt(12)
 * One wave per frame, float32 sums (lane-strided partial sums, then one butterfly over the wave); columns F .. ld-1 are never
 * read.  DCS_EINVAL for F < 1, ld < F, n_frames < 0, a negative or NaN floor, a class outside -1 .. 11 or a NULL pointer;
 * n_frames == 0 does nothing.  Enqueued on the ctx stream. */
DCS_API int dcs_chroma(dcs_ctx* ctx, const float* mag_d, int64_t ld, int64_t n_frames, int F, const int8_t* cls_h, float floor,
                       float* chroma_d);
/* Dynamic time warping of a_d [T][12] (audio) onto s_d [U][12] (score), float32 throughout:
 *   c[t,u] = 1 - sum_k a[t,k] s[u,k]  (twelve fused multiply-adds, then one subtraction)
 *   D[0,0] = c[0,0];  D[t,u] = c[t,u] + best, rounded once, where best = D[t-1,u-1] (code 0), replaced by D[t-1,u] (code 1)
 *   only if that is strictly smaller, then by D[t,u-1] (code 2) only if that is strictly smaller than the best so far;
 *   neighbours outside the matrix are +inf.
 * band >= 0: cell (t, u) is in the band iff |u (T-1) - t (U-1)| <= band (T-1) (int64), every other cell is +inf; band == -1:
 * no band.  Outputs on the device: path_d [T+U-1][2] int32, rows 0 .. n-1 the cells (t, u) from (0, 0) to (T-1, U-1) in forward
 * order (the rows behind them are not written), *n_path_d = n (int64), *cost_d = D[T-1,U-1]; when the end cell is +inf, n = 0
 * and the cost +inf.  Tiles of dcs_dtw_tile() x dcs_dtw_tile() cells, one wave each, lane = row, columns walked skewed; ONE
 * launch per anti-diagonal of tiles, ordered by the stream (no kernel waits for another workgroup), tiles wholly outside the
 * band are not launched; then one launch with a single walker, a counted loop of at most T + U - 1 steps.  1 + ceil(T / tile) +
 * ceil(U / tile) - 1 + 1 launches without a band.  Scratch -- the strips between tiles, the path from the back, 2 bits per cell
 * of the tiles that touch the band, so about T min(U, 2 band + tile) / 4 bytes -- comes from the context's workspace;
 * dcs_dtw_bytes reports it (-1 where dcs_dtw would refuse the shape).  DCS_EINVAL for T or U < 1, band < -1, a NULL pointer, or
 * a band that cannot hold a path: 2 band + 1 < ceil((U-1) / max(T-1, 1)).  DCS_ESHAPE for T or U above 2^20 or scratch above
 * 2 GiB.  A refused call writes nothing.  Enqueued on the ctx stream; nothing of size T x U leaves the device. */
DCS_API int dcs_dtw_tile(void);
DCS_API int64_t dcs_dtw_bytes(int64_t T, int64_t U, int64_t band);
DCS_API int dcs_dtw(dcs_ctx* ctx, const float* a_d, int64_t T, const float* s_d, int64_t U, int64_t band, int32_t* path_d,
                    int64_t* n_path_d, float* cost_d);

/* ------------------------------------------------------------------ score following (csrc/follow.hip) */
/* dcs_dtw on a stream: a score follower with constant memory.  It takes chroma rows of the audio as they arrive and returns,
 * for each, the score frame the performance has reached.  Nothing of size T x U exists anywhere; a push allocates nothing and
 * never waits for the device; all state is a function of (U, W, max_frames).  All arithmetic is float32 and every operation
 * is rounded once.  State and parameters:
 *   the score S[U][12], uploaded once at creation;  the window width W, a multiple of 64, 64 <= W <= 1024;  K, the largest
 *   number of score frames one audio frame may advance, 1 <= K <= 4;  back, the cells kept behind the position, 0 <= back < W;
 *   lambda, the penalty on a step other than 1, finite and >= 0;  window start w0 = 0, position p = 0, frame count t = 0;
 *   one row D[u] over the window w0 <= u < min(U, w0 + W), every other cell +inf.
 * For audio frame t with chroma row a:
 *   c[u] = 1 - sum_k a[k] S[u][k] for u in the window (dcs_dtw's cost: twelve fused multiply-adds in the order k = 0 .. 11,
 *   then one subtraction)
 *   t == 0:  D'[0] = c[0], every other cell +inf: the follower starts at the score's first frame
 *   t > 0:   best[u] = min(D[u-1], D[u] + lambda, D[u-k] + lambda for k = 2 .. K), cells below w0 and u - k < 0 being +inf;
 *            D'[u] = c[u] + best[u]
 *   m = min_u D'[u], q = the lowest u that attains it;  p = max(p, q);  D[u] = D'[u] - m (the row stays bounded on a stream
 *   of any length);  pos[t] = p
 *   the window moves: w0 = max(w0, max(0, min(q - back, U - W))) -- only forward, tied to q and not p, so that the minimum's
 *   cell is always inside and m always finite; cells that enter are +inf.
 * Every audio frame takes exactly one step, so all cells of a row have paths of equal length: no normalisation, and a row has
 * no dependence along u.  One launch per push, one workgroup of W threads, the frames of the push in a loop counted by n; the
 * result does not depend on how the frames are cut into pushes.
 * dcs_follow_push: chroma_d [n][12] (dcs_chroma's rows), pos_d [n] int32, 0 <= n <= max_frames (n == 0 does nothing), enqueued
 * on the ctx stream.  dcs_follow_reset starts another signal and keeps the score.  dcs_follow_frames is the host's count of
 * frames pushed since create or reset.  dcs_follow_row copies the state out, device to device: row_d [W] with cell w0 + i at i,
 * +inf past U (all +inf before the first frame), *w0_d (int64), *p_d (int32).  DCS_EINVAL for the parameter ranges above, U < 1,
 * max_frames < 1, a NULL pointer, a lambda that is not finite, n < 0 or n > max_frames; DCS_ESHAPE for U above 2^30 or
 * max_frames above 2^31 - 1.  A refused call writes nothing and leaves the state as it was.  Not followed: a performance that
 * goes back, one that starts anywhere but at the score's first frame, one faster than K times nominal tempo. */
typedef struct dcs_follow dcs_follow;
DCS_API int dcs_follow_create(dcs_ctx* ctx, const float* s_h, int64_t U, int W, int K, int back, float lambda, int64_t max_frames,
                              dcs_follow** out);
DCS_API int dcs_follow_destroy(dcs_follow* f);
DCS_API int dcs_follow_reset(dcs_follow* f);
DCS_API int64_t dcs_follow_bytes(const dcs_follow* f);  /* -1 for NULL */
DCS_API int64_t dcs_follow_frames(const dcs_follow* f); /* -1 for NULL */
DCS_API int dcs_follow_push(dcs_follow* f, const float* chroma_d, int64_t n, int32_t* pos_d);
DCS_API int dcs_follow_row(dcs_follow* f, float* row_d, int64_t* w0_d, int32_t* p_d);

/* ------------------------------------------------------------------ multichannel Wiener filter (csrc/mwf.hip) */
/* The filter the reference's authors were transcribing behind their stereo network and never ran: util.py:633-719 mwf(spec,
 * mixture, niter=10) quotes the MATLAB of Duong / Vincent / Gribonval's EM for full-rank spatial covariances (:647-682), stops
 * at a pdb.set_trace() (:718) and its update line (:719) has inconsistent dimensions.  What runs here is that EM with gamma1 =
 * 0 (no temporal prior) and a time-invariant spatial covariance R_j[f], for I = 2 channels and J sources:
 *   X[c,t,f] = mag[c,t,f] e^{i phase[c,t,f]},   A[c,j,t,f] = src[c,j,t,f] / pre_div  (float32 division)
 *   init:   y_j[t,f] = (A[0,j] e^{i phase[0]}, A[1,j] e^{i phase[1]}),  C_j = y_j y_j^H,  v_j = tr(C_j) / 2
 *   niter times:
 *     M:    R_j[f] = sum_t C_j[t,f] / (sum_t v_j[t,f] + eps)
 *     E:    Cx = sum_j v_j R_j + eps I,  W_j = v_j R_j Cx^{-1},  y_j = W_j x,
 *           C_j = y_j y_j^H + (I - W_j) v_j R_j,  v_j = Re tr(C_j) / 2
 *   out:    |y_j[c]|, angle(y_j[c]) (0 where y is 0), float32
 * niter = 0 returns src / pre_div and the mixture's phases.  mag_d / phase_d [2][n_frames, ld] (channel stride ch_stride);
 * src_d, out_mag_d, out_phase_d [2][J][n_frames, ld] (strides src_ch_stride, src_stride, in elements, shared by all three);
 * columns F .. ld-1 of the outputs are not written.  pre_div: the scale_factor the stereo path's magnitudes carry (as in
 * dcs_stft_inverse_f32).  The 2x2 algebra, the phasors and the sums over t are float64, what is kept between passes (v_j
 * [J][n_frames][F]) float32 in the context's scratch; one launch per pass, niter + 1 launches, no atomics: the same bits every
 * run.  DCS_EINVAL for J outside 1 .. 8, niter outside 0 .. 100, F < 1, ld < F, pre_div <= 0, eps <= 0 (or below DBL_MIN:
 * the inverse of an empty bin's Cx = eps I must be finite; any normal eps keeps zero rows at zero) or a NULL pointer;
 * n_frames == 0 does nothing.  Enqueued on the ctx stream. */
DCS_API int dcs_mwf_f32(dcs_ctx* ctx, const float* mag_d, const float* phase_d, int64_t ch_stride, const float* src_d,
                        int64_t src_ch_stride, int64_t src_stride, int64_t ld, int64_t n_frames, int F, int J, int niter,
                        float pre_div, double eps, float* out_mag_d, float* out_phase_d);
/* frames of one chunk of dcs_mwf_f32: a workgroup sums over one chunk, or over every 32nd one past 32 chunks, and the next
 * pass adds up min(ceil(n_frames / this), 32) sets of sums */
DCS_API int dcs_mwf_frames_per_block(void);

/* The same filter on a stream (csrc/mwf_online.hip): a causal form whose state per (source, bin) is one Hermitian 2x2 matrix,
 * S_j[f], four float64 -- constant memory however long the signal is.  X and A as in dcs_mwf_f32; every bin f is independent,
 * t is the ABSOLUTE frame since create or reset:
 *   init:   y_j = (A[0,j] e^{i phase[0]}, A[1,j] e^{i phase[1]}),  C_j = y_j y_j^H,  v_j = tr(C_j) / 2
 *           G_j = forget * S_j[t-1]              (zero at t = 0: the state is NOT read for frame 0)
 *   niter times:
 *           N_j = G_j + C_j,   n_j = Re tr(N_j) / 2
 *           R_j = (N_j + loading n_j I) / ((1 + loading) n_j + eps)
 *           Cx  = sum_j v_j R_j + eps I  (j increasing),   W_j = v_j R_j Cx^{-1},   y_j = W_j x
 *           C_j = y_j y_j^H + (I - W_j) v_j R_j,   v_j = Re tr(C_j) / 2
 *   after:  S_j[t] = G_j + C_j
 *   out:    |y_j[c]|, angle(y_j[c]) (0 where y is 0), float32
 * R_j is the running (forget < 1: exponentially forgetting) average of the posterior covariances of the frames so far and of
 * THIS frame's current one, normalised to unit mean trace; `loading` adds that fraction of an isotropic covariance, without
 * which frame 0 has a rank-1 R_j and, where every estimate is a mask times the same mixture, a Cx singular up to eps.  It is
 * NOT the batch filter and is not expected to match it: the first frames of a signal are filtered on little evidence.
 * niter = 0 returns src / pre_div and the mixture's phases bit for bit and keeps no state.  Phasors, 2x2 algebra and state are
 * float64, inputs and outputs float32; v_j never leaves registers.  A push filters the absolute frames frames .. frames +
 * n_frames - 1 and advances the count: ONE launch on the ctx stream, one lane per bin with the J sources in registers, time
 * serial, every sum in a fixed order, no atomics -- the same bits every run and however the frames are cut into pushes.
 * Layouts and strides are those of dcs_mwf_f32; columns F .. ld-1 of the outputs are not written.  reset sets the count to 0
 * and touches no device memory; bytes (the state, [J][4][F] float64 rounded up to 256 bytes) depends on (F, J) alone.
 * DCS_EINVAL for J outside 1 .. 8, niter outside 0 .. 100, F < 1, ld < F, forget outside (0, 1], loading negative or not finite,
 * eps <= 0 or below DBL_MIN, pre_div <= 0, n_frames < 0, a stride below n_frames * ld, or a NULL pointer; n_frames == 0 does
 * nothing. */
typedef struct dcs_mwf_online dcs_mwf_online;
DCS_API int dcs_mwf_online_create(dcs_ctx* ctx, int F, int J, int niter, double forget, double loading, double eps,
                                  dcs_mwf_online** out);
DCS_API int dcs_mwf_online_destroy(dcs_mwf_online* h);
DCS_API int dcs_mwf_online_reset(dcs_mwf_online* h);
DCS_API int64_t dcs_mwf_online_bytes(const dcs_mwf_online* h);  /* -1 for NULL */
DCS_API int64_t dcs_mwf_online_frames(const dcs_mwf_online* h); /* frames pushed since create or reset; -1 for NULL */
DCS_API int dcs_mwf_online_push_f32(dcs_mwf_online* h, const float* mag_d, const float* phase_d, int64_t ch_stride,
                                    const float* src_d, int64_t src_ch_stride, int64_t src_stride, int64_t ld, int64_t n_frames,
                                    float pre_div, float* out_mag_d, float* out_phase_d);

/* ------------------------------------------------------------------ per-channel masks of the mono models (csrc/chanmask.hip) */
/* Every published model but the ILD one sees a mono down-mix (separate_dsd.py:285-287, separate_ikala.py:229) and the scripts
 * write mono stems.  This applies the network's soft masks (separate_dsd.py:258-271, separate_bach10.py:251-264), cross-faded
 * over the tiles as overlapadd_multi stitches them (util.py:297-327), to the magnitudes of EACH input channel: the estimates a
 * per-channel iSTFT -- or first dcs_mwf_f32, the filter of util.py:633-719 -- turns into stereo stems.  Per frame t, bin f:
 *   per covering tile k (frame j = t - k st of it, st = time_context - overlap), float32, eps_r = 5e-19f:
 *     DCS_EPS_A:  q_s = p_s + eps_r,  den = ((q_0 + q_1) + ...),  m_s = q_s / den
 *     DCS_EPS_B:  den = ((p_0 + p_1) + ...) + eps_r,              m_s = p_s / den
 *   the fold of dcs_overlap_add on the masks: owner tile k0 = t < overlap ? 0 : min((t - overlap) / st, n_tiles - 1), acc = m[k0],
 *     then for increasing k > k0 with k st <= t:  acc = fma(rise[overlap - 1 - j], acc, rise[j] * m[k])  (the product rounded)
 *   mask_d[s][t, f] = acc_s,   est_d[c][s][t, f] = acc_s * mag_d[c][t, f]
 * p_d: the rectified network output as dcs_model_forward leaves it, element (s, k, j, f) at p_d + s p_src_stride + (k
 * time_context + j) F + f (the stride lets S < channels_out through); rise_h = np.linspace(0, 1, overlap) as float64, as for
 * dcs_overlap_add; mag_d [C][n_frames, ld] (channel stride mag_ch_stride), scaled however the caller likes; est_d
 * [C][S][n_frames, ld] (strides est_ch_stride, est_src_stride) and mask_d [S][n_frames, ld] (stride mask_src_stride), either may be
 * NULL.  Rows past the last tile (t - k0 st >= time_context; every row when n_tiles == 0) are written as zeros, columns
 * F .. ld-1 are never written.  One launch, no atomics: the same bits every run.  DCS_EINVAL for S or C outside 1 .. 8, overlap
 * outside 1 .. time_context - 1, F < 1, ld < F, a negative count, an eps_mode that is neither convention, a NULL p_d, mag_d or
 * rise_h, or both outputs NULL; n_frames == 0 does nothing.  Enqueued on the ctx stream (a ramp whose values differ from the
 * previous call's is uploaded first, after a stream synchronisation, as in dcs_overlap_add). */
DCS_API int dcs_mask_fold_apply(dcs_ctx* ctx, const float* p_d, int64_t p_src_stride, int64_t n_tiles, int S, int time_context,
                                int overlap, int F, int eps_mode, const double* rise_h, const float* mag_d, int64_t mag_ch_stride,
                                int C, int64_t n_frames, int64_t ld, float* est_d, int64_t est_ch_stride, int64_t est_src_stride,
                                float* mask_d, int64_t mask_src_stride);

/* ------------------------------------------------------------------ streaming separation (csrc/stream.hip) */
/* Every path above separates a signal that is complete and resident.  A stream takes the signal in blocks and hands back the
 * samples of the SAME whole-file computation (stft_norm -> tiler -> network -> the fold of dcs_mask_fold_apply -> istft_norm) as
 * soon as no later input can change them, in memory that does not depend on the signal's length.  With N = frameSize, h = hop,
 * H = N / 2, st = time_context - overlap, P samples pushed so far and, once the signal has ended, L samples in all -- host
 * integers, no call waits for the device to know them:
 *   complete frames  A = P < H ? 0 : (P - H) / h + 1          after the end  T = dcs_frame_count(L, h)
 *   ready tiles      K = A < tc ? 0 : (A - tc) / st + 1                      dcs_tile_count(T, tc, overlap, tiler)
 *   folded frames    Tf = K st                                               T
 *   emitted samples  E = max(0, Tf h - H)                                    L
 * Frame n covers samples [n h - H, n h - H + N); samples < 0 and >= L read as zero.  Mid-stream E > P - tc h - N once A >= tc.
 *   frames  mag[n][f] = |rfft(w frame_n)| / sqrt(N), phase = angle(.), as dcs_stft_forward_f32
 *   tiles   tiles[k][0][j][f] = scale * mag[k st + j][f], zero for rows >= T
 *   fold    est[s][t][f] = acc_s[t][f] * mag[t][f]: the per-frame definition of dcs_mask_fold_apply on the UNSCALED
 *           magnitudes (pre_div = 1), n_tiles = the tiles so far (mid-stream the owner of a folded frame is always below it)
 *   inverse y_n = w * irfft(est[s][n] sqrt(N) exp(j phase[n])),  out[s][q] = (y_lo[..] + y_lo+1[..] + ... in increasing n) / norm(q)
 *           over the frames n < Tf with n h <= q + H < n h + N, norm = the sum of w^2 over the same frames, 0 replaced by 1
 * float32 on the device, no atomics, every kernel a pure function of absolute sample / frame / tile indices: the bits that come
 * out do not depend on how the signal is cut into blocks.
 * Supported: N % h == 0 (else DCS_EUNSUPPORTED), h <= N / 2, N >= 64, 1 <= overlap < time_context, S in 1 .. 8, a known tiler
 * and eps_mode, 1 <= max_push <= 2^30 (else DCS_EINVAL); one signal channel (dcs_stream_create_channels below: several).  rise_h as for dcs_overlap_add.  All state -- a
 * ring of N + max_push samples, rings of magnitude / phase rows, of p for the last ceil(tc / st) tiles plus one push's, of
 * windowed time-domain frames [N / h + frames per pull][S][N], the estimates of one pull -- is allocated by create; its size is a
 * function of (N, h, tc, overlap, S, max_push) alone, push and pull allocate nothing.  No ring slot is read before the push or
 * pull that needs it has written it, so create and reset initialise nothing.  The plan must outlive the stream. */
typedef struct dcs_stream dcs_stream;
DCS_API int dcs_stream_create(dcs_stft* plan, int S, int time_context, int overlap, int tiler, int eps_mode, float scale,
                              const double* rise_h, int64_t max_push, dcs_stream** out);
DCS_API int dcs_stream_destroy(dcs_stream* s);
/* back to the empty state (P = 0, not ended); nothing is reallocated */
DCS_API int dcs_stream_reset(dcs_stream* s);
/* the most tiles one push can return, the end included; the device bytes the stream holds */
DCS_API int64_t dcs_stream_max_tiles(const dcs_stream* s);
DCS_API int64_t dcs_stream_bytes(const dcs_stream* s);
/* Appends audio_d[0 .. n), 0 <= n <= max_push; last != 0 ends the signal (n == 0 is fine).  Transforms the frames that became
 * complete -- mag_d / phase_d [n_frames, ld], either may be NULL, receive their rows, columns past the bins zero -- and writes the
 * tiles that became ready, tiles_d [n_tiles, 1, time_context, N / 2 + 1] (tiles_cap: the tiles it has room for).  The counts
 * returned are the formulas above.  Enqueued on the ctx stream of the plan. */
DCS_API int dcs_stream_push(dcs_stream* s, const float* audio_d, int64_t n, int last, float* tiles_d, int64_t tiles_cap,
                            int64_t* n_tiles_out, float* mag_d, float* phase_d, int64_t ld, int64_t* n_frames_out);
/* p_d: the first S channels of what dcs_model_forward wrote for EXACTLY the tiles of the preceding push, element (s, k, j, f)
 * at p_d + s p_src_stride + (k time_context + j) (N / 2 + 1) + f.  Folds the frames no later tile can reach -- est_d
 * [S][n rows, ld] (source stride est_src_stride), may be NULL, receives their estimates -- inverts them and writes the samples
 * that became final, pcm_d [S][n_out] (source stride pcm_stride, room for pcm_cap samples per source).  Pushes and pulls
 * alternate strictly: a pull with another tile count than the push returned, a pull without a push, two pushes in a row or a
 * push after the end give DCS_EINVAL.  An ended signal that yields no tile at all makes the last pull fail with DCS_EINVAL, as
 * dcs_separate fails. */
DCS_API int dcs_stream_pull(dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t n_tiles, float* pcm_d,
                            int64_t pcm_stride, int64_t pcm_cap, int64_t* n_out, float* est_d, int64_t est_src_stride,
                            int64_t ld);
/* A CHANNEL stream: C signal channels (1 <= C <= 8, the range of dcs_mask_fold_apply) next to the down-mix the network sees,
 * for stems per channel from the mono models -- the masks of the down-mix on every channel's own magnitudes with its own phase,
 * as Separator.separate_channels computes them on a whole file.  The schedule, the counts, the refusals and the invariants are
 * the mono stream's; the kernels are the same ones with a row / channel index, every expression term for term.  State: sample
 * rings (C + 1)(N + max_push), magnitude rows (C + 1) rf F, phase rows C rf F, estimates C S ff F, time frames rt C S N, the
 * ring of p ONCE (rf = ff = tc + fp, fp = ceil((max_push + H) / h) + 3, rt = N / h + ff): a function of (N, h, tc, overlap,
 * S, C, max_push) alone.  destroy, reset, max_tiles and bytes are dcs_stream's.  dcs_stream_push / _pull on a channel stream and
 * the two calls below on a mono stream give DCS_EINVAL. */
DCS_API int dcs_stream_create_channels(dcs_stft* plan, int S, int C, int time_context, int overlap, int tiler, int eps_mode,
                                       float scale, const double* rise_h, int64_t max_push, dcs_stream** out);
/* audio_d: C + 1 rows of n samples, row r at audio_d + r row_stride (>= n): rows 0 .. C - 1 the channels, row C the down-mix,
 * which the caller forms (so the network's input is that of the mono stream on the same down-mix, bit for bit).  All rows go
 * into their rings and are transformed; the tiles come from the down-mix row alone.  mag_d / phase_d [C][n_frames, ld] (channel
 * stride ch_stride >= n_frames ld, either may be NULL) receive the CHANNELS' rows. */
DCS_API int dcs_stream_push_channels(dcs_stream* s, const float* audio_d, int64_t row_stride, int64_t n, int last,
                                     float* tiles_d, int64_t tiles_cap, int64_t* n_tiles_out, float* mag_d, float* phase_d,
                                     int64_t ch_stride, int64_t ld, int64_t* n_frames_out);
/* p_d as for dcs_stream_pull; it goes into its ring once and one fold per (frame, bin) computes acc_s, then
 * est[c][s][t][f] = acc_s[t][f] * mag[c][t][f] for every channel.  One inverse per (frame, channel, source) with that channel's
 * phase; pcm_d [C][S][n_out] (element (c, s, i) at pcm_d + c pcm_ch_stride + s pcm_stride + i), est_d [C][S][rows, ld] (channel
 * stride est_ch_stride, source stride est_src_stride; may be NULL).  Strides below the counts give DCS_EINVAL. */
DCS_API int dcs_stream_pull_channels(dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t n_tiles, float* pcm_d,
                                     int64_t pcm_ch_stride, int64_t pcm_stride, int64_t pcm_cap, int64_t* n_out, float* est_d,
                                     int64_t est_ch_stride, int64_t est_src_stride, int64_t ld);
/* A STEREO stream: the stereo (ILD) graph, whose network sees the C channels themselves (1 <= C <= 8; the published graph has
 * C = 2) and returns one output per (source, channel).  There is no down-mix row.  The schedule, the counts, the refusals and
 * the invariants are the mono stream's; frames, inverse and gather are the same kernels with a channel index.
 *   tiles   the row layout dcs_model_forward_stereo takes: tiles[k][j][c][f] = scale * mag[c][k st + j][f], zero for rows >= T
 *           and for the columns F .. ld_t - 1, ld_t = F rounded up to 4
 *   fold    per frame t, bin f, channel c, float32, eps_r = 1e-13f (1e-12 x 0.1, trainCNN_ILD_DSD100.py:152,164,187), every
 *           sum, quotient and product rounded once, in the order written:
 *             per covering tile k (row j = t - k st):  den = (((p_0c + p_1c) + ...) + eps_r,  m_s = p_sc / den
 *             acc_sc: the fold of dcs_mask_fold_apply on m (owner tile k0, then fma(rise[ov-1-j], acc, rise[j] * m[k]))
 *             est[c][s][t][f] = acc_sc * mag[c][t][f] + c0,   c0 = eps_r / scale formed once, by create, in float32
 *           on the UNSCALED magnitudes: the cross-fade of mask * (scale * mag) + eps_r (:188) divided by scale, as the weights
 *           of a frame sum to one -- dcs_separate_stereo's result in exact arithmetic.  Rows past the last tile are exact
 *           zeros, without c0 (util.py:313).
 * State: sample rings C (N + max_push), magnitude rows C rf F, phase rows C rf F, the ring of p S C rp tc F (every (source,
 * channel) once), estimates C S ff F, time frames rt C S N, the ramp (rf = ff = tc + fp, fp = ceil((max_push + H) / h) + 3,
 * rp = ceil(tc / st) + max_tiles, rt = N / h + ff): a function of (N, h, tc, overlap, S, C, max_push) alone.  destroy, reset,
 * max_tiles and bytes are dcs_stream's.  The mono, channel and score calls on a stereo stream and the three calls below on any
 * other stream give DCS_EINVAL; scale == 0 gives DCS_EINVAL. */
DCS_API int dcs_stream_create_stereo(dcs_stft* plan, int S, int C, int time_context, int overlap, int tiler, float scale,
                                     const double* rise_h, int64_t max_push, dcs_stream** out);
/* audio_d: C rows of n samples, row c at audio_d + c row_stride (>= n).  mag_d / phase_d [C][n_frames, ld] (channel stride
 * ch_stride >= n_frames ld, either may be NULL); tiles_d [n_tiles][time_context][C][ld_t]. */
DCS_API int dcs_stream_push_stereo(dcs_stream* s, const float* audio_d, int64_t row_stride, int64_t n, int last, float* tiles_d,
                                   int64_t tiles_cap, int64_t* n_tiles_out, float* mag_d, float* phase_d, int64_t ch_stride,
                                   int64_t ld, int64_t* n_frames_out);
/* p_d for EXACTLY the tiles of the preceding push, element (s, c, k, j, f) at p_d + s p_src_stride + c p_ch_stride + (k
 * time_context + j) p_ld + f: dcs_model_forward_stereo's output has p_src_stride = n tc C ld_t, p_ch_stride = ld_t, p_ld = C
 * ld_t; the Lasagne layout [S C][n][tc][F] has p_src_stride = C n tc F, p_ch_stride = n tc F, p_ld = F.  p_ld < F, a source
 * stride below one source's extent, or channels that are neither whole planes (p_ch_stride >= the rows' extent) nor side by
 * side in a row (p_ld >= (C - 1) p_ch_stride + F) give DCS_EINVAL.  p goes into its ring once.  One inverse per (frame,
 * channel, source) with that channel's phase; pcm_d [C][S][n_out], est_d [C][S][rows, ld] as for dcs_stream_pull_channels. */
DCS_API int dcs_stream_pull_stereo(dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t p_ch_stride, int64_t p_ld,
                                   int64_t n_tiles, float* pcm_d, int64_t pcm_ch_stride, int64_t pcm_stride, int64_t pcm_cap,
                                   int64_t* n_out, float* est_d, int64_t est_ch_stride, int64_t est_src_stride, int64_t ld);
/* A SCORE stream: the score-informed graphs (dcs_model_forward's [n, ninst, tc, F] tiles) on a stream.  The score is known
 * before the audio: notes_h [ninst][n_notes][width] is the table dcs_score_masks takes, read by the rules of that call -- a row
 * counts if midi > 0 and its duration n1 - max(n0, 0) is positive, it covers the frames (int64)max(n0, 0) <= t < (int64)n1; a
 * pair (fs, fe) counts if fe > 0 and covers the bins (int64)fs <= f < (int64)fe; width >= 5 and odd (else DCS_EINVAL); a bin
 * range outside [0, F) gives DCS_ESHAPE.  1 <= ninst <= 8, normalise DCS_SCORE_NORM_MAX | _SUM, mixture DCS_MIX_CH0 | _SUM in
 * any combination (else DCS_EINVAL); everything else as dcs_stream_create refuses it.  The table is converted (rows sorted by
 * first frame, with the running maximum of their end frames, so that a push looks only at the rows that can meet its frames) and
 * uploaded once, here; push and pull still allocate nothing and never wait for the device.  All arithmetic float32, every
 * product, sum and quotient below rounded once, in the order written:
 *   mask    for absolute frame t, instrument j, bin f:  on_j[t][f] = some counting row of j covers t and one of its counting
 *           pairs covers f -- filterSpec with the window (0, +inf); rows t >= T never reach a tile (the tiler's zeros)
 *     DCS_SCORE_NORM_MAX  M_j = on_j ? hi_j : lo_j,  hi_j = 1 / max_j,  lo_j = 1e-18f / max_j,  max_j = 1 if instrument j has any
 *                         non-empty rectangle (frames and bins) in the table AS GIVEN, else 1e-18f (such an instrument: all ones)
 *     DCS_SCORE_NORM_SUM  v_i = on_i ? 1 : 1e-18f,  total = ((v_0 + v_1) + ...),  M_j = v_j / total  (score_sumnorm_kernel's)
 *           The one difference from dcs_score_masks_norm(.., start = 0, stop = n_frames, ..): there "any rectangle" and the
 *           clip of a row are taken against stop = n_frames, here against +inf.  The two agree whenever no note row ends past
 *           the signal's frame count (a row that only BEGINS there is the case that differs: it makes max_j = 1 here), which
 *           holds for a table built by melody_table(..., nframes = T).
 *   tiles   tiles[k][j][r][f] = M_j[t][f] * (scale * mag[t][f]),  t = k st + r,  zero for t >= T  (score_floor_kernel's product)
 *   fold    est[s][t][f] = acc_s[t][f] * mix[t][f], acc_s exactly as in the mono stream, on the UNSCALED magnitudes (pre_div = 1):
 *     DCS_MIX_CH0  mix = M_0 * mag        DCS_MIX_SUM  mix = ((x_0 + x_1) + ...),  x_j = M_j * mag
 *   inverse, gather, schedule, counts, refusals: the mono stream's.
 * dcs_stream_push / _pull / _reset / _destroy / _max_tiles / _bytes work on such a stream; tiles_d is [n_tiles, ninst,
 * time_context, F]; reset keeps the score; dcs_stream_push_channels / _pull_channels give DCS_EINVAL.  State: the mono stream's
 * plus a ring of mask rows [ninst][rf][F] (written by the push that completes a frame, next to its magnitudes) and the converted
 * table (ninst n_notes rows of 4 + (width - 3) int32): dcs_stream_bytes is a function of (N, h, tc, overlap, S, ninst, n_notes,
 * width, max_push) alone. */
DCS_API int dcs_stream_create_score(dcs_stft* plan, int S, int time_context, int overlap, int tiler, int eps_mode, float scale,
                                    const double* rise_h, int64_t max_push, const double* notes_h, int ninst, int n_notes,
                                    int width, int normalise, int mixture, dcs_stream** out);

/* The multichannel Wiener filter on a channel or stereo stream of C == 2 channels: the online filter of dcs_mwf_online_* (J = S
 * sources, its state in the stream).  Called before the first push, or after a reset; niter = 0 turns the filter off again.
 * With it on, a pull runs the fold as before, then the filter over exactly the rows this pull folded -- X from the magnitude and
 * phase rings, A = the fold's estimates, pre_div = 1 -- into two buffers [C][S][ff][F] of filtered magnitudes and phases, then
 * the inverse on THOSE (a phase per (channel, source)), then the gather.  est_d of the pull still receives the unfiltered
 * estimates; dcs_stream_mwf_last copies out the filtered rows of the last pull, mag_d / phase_d [C][S][rows, ld] (strides in
 * elements; rows = the frames that pull folded; columns past the bins are not written).  The filter is causal and its bits do
 * not depend on the cut, so the stream keeps its contract; it is not the batch filter of dcs_mwf_f32 and the first frames of a
 * signal are filtered on little evidence.  dcs_stream_bytes grows by the two buffers and dcs_mwf_online_bytes -- a function of
 * the shapes alone -- and a stream whose filter was never armed allocates, launches and computes what it did without it.
 * DCS_EINVAL for a mono or score stream, C != 2, a stream that has samples, or values dcs_mwf_online_create refuses;
 * dcs_stream_mwf_last: the filter off, a NULL buffer, ld below the bins or strides below the rows. */
DCS_API int dcs_stream_set_mwf(dcs_stream* s, int niter, double forget, double loading, double eps);
DCS_API int dcs_stream_mwf_last(dcs_stream* s, float* mag_d, float* phase_d, int64_t ch_stride, int64_t src_stride, int64_t ld);

/* A FOLLOWED score stream: the score is at nominal tempo and a follower (dcs_follow_*, above) says where in it the performance
 * is.  The note table of such a stream is in SCORE time -- melody_table at nominal tempo with nframes = U -- a position is a
 * frame index into that table, and the stream's hop is the follower's hop.  Called on a score stream before the first push;
 * cls_h [F] and floor are dcs_chroma's (uploaded once, here).  Armed, a push runs on the stream's queue, in this order: the
 * frames, as before; dcs_chroma's kernel on the new magnitude rows (in two pieces where the ring wraps); the follower's push;
 * then, instead of the mask kernel of the unfollowed stream, one that paints audio frame t from score frame pos[t] and looks at
 * every row of the table (the host no longer knows which rows a push can meet).  Tiles, fold, inverse and gather read the mask
 * ring as before, and a stream that was never armed allocates, launches and computes what it did without this call.
 * dcs_stream_reset resets the follower too.  A push that fails with a HIP error after the follower has taken its frames leaves
 * the follower ahead of the stream: every later push is refused (DCS_EINVAL) until dcs_stream_reset.  dcs_stream_bytes grows by the position and chroma buffers (a push's frames) and the
 * class table; the follower's own bytes are dcs_follow_bytes.  The follower stays the caller's: it must outlive the stream's
 * pushes and is not destroyed with the stream.  dcs_stream_follow_last copies the positions of the last push into pos_d [cap]
 * (device) and stores their count in *n (host).  DCS_EINVAL: s is not a score stream; the stream or the follower has already
 * taken frames; the follower's max_frames is below the frames one push of the stream can complete; another context's follower; a
 * class outside -1 .. 11, a negative or NaN floor, a NULL pointer; dcs_stream_follow_last: a stream that is not armed, cap below
 * the count, a NULL pointer. */
DCS_API int dcs_stream_set_follow(dcs_stream* s, dcs_follow* f, const int8_t* cls_h, float floor);
DCS_API int dcs_stream_follow_last(dcs_stream* s, int32_t* pos_d, int64_t cap, int64_t* n);

/* ------------------------------------------------------------------ sample-rate conversion (csrc/resample.hip) */
/* The reference separates 44 100 Hz files only (separate_dsd.py:283 prints "Sample rate is not 44100" for the rest); this is
 * the rate change in front of the STFT and behind the iSTFT that lets every other file through.  For up / down = fo / fi in
 * lowest terms and a filter h[t], t = -half .. half, on the grid of rate up * fi (designed on the host in float64,
 * deepconvsep_amd/resample.py: Kaiser-windowed sinc, cut-off rolloff * min(fi, fo) / 2):
 *   y[m] = sum_n x[n] h[m down - n up],   0 <= n < n_in,  |m down - n up| <= half,   m = 0 .. ceil(n_in up / down) - 1
 * (scipy.signal.resample_poly(x, up, down, window=h / up)): x is zero outside [0, n_in), the filter is centred, no delay. */
typedef struct dcs_resampler dcs_resampler;
/* ceil(n_samples * up / down); -1 for n_samples < 0, up < 1, down < 1 or a product past int64 */
DCS_API int64_t dcs_resample_length(int64_t n_samples, int up, int down);
/* taps_h: the 2 half + 1 values of h (host, float64).  They are stored as float32, one row per phase p = (m down) mod up
 * holding that phase's taps h[p + j up] in the order the kernel adds them (ascending n).  DCS_EINVAL for up < 1, down < 1,
 * half < 0 (checked before anything else) or a NULL pointer.  DCS_EUNSUPPORTED for what the plan cannot hold: up or down above
 * 2^20; a table of up x round_up(2 half / up + 1, 4) float32 above 1 MiB (32 zero crossings at rolloff 0.95 need 43 KB for
 * 160/147, 44 KB for 147/160, 85 KB for 147/320, 117 KB for 441/320, 441/160 and 441/80); 256 consecutive outputs reaching over more than 64 KiB of input
 * (256 down / up + 2 half / up samples).  Synchronous (two small uploads). */
DCS_API int dcs_resample_plan(dcs_ctx* ctx, int up, int down, const double* taps_h, int64_t half, dcs_resampler** out);
DCS_API int dcs_resample_plan_destroy(dcs_resampler* r);
/* n_clips signals of n_in float32 samples, signal k at in_d + k in_stride, -> dcs_resample_length(n_in, up, down) samples each
 * at out_d + k out_stride (strides in elements, at least the lengths when n_clips > 1), ONE launch.  Nothing outside [in_d + k
 * in_stride, + n_in) is read and nothing outside the outputs written.  Float32 arithmetic: every output is one fmaf chain over
 * its taps in ascending n -- the order depends on (up, down, half) only, so a batched call, a single one and a longer signal
 * with the same samples under the window give the same bits.  n_in == 0 or n_clips == 0 does nothing.  Enqueued on the ctx
 * stream of the plan. */
DCS_API int dcs_resample_f32(dcs_resampler* r, const float* in_d, int64_t n_in, int64_t n_clips, int64_t in_stride,
                             float* out_d, int64_t out_stride);
/* The same conversion of a signal that arrives in blocks: `rows` signals (1 .. 64) in lock-step on a plan, which must outlive the
 * stream.  Output m touches inputs ceil((m down - half) / up) .. floor((m down + half) / up), so after P samples mid-stream
 *   M(P) = P up - 1 - half < 0 ? 0 : (P up - 1 - half) / down + 1
 * outputs are final (every tap below P), after the end ceil(L up / down); an output not yet emitted reaches back less than
 * 2 half / up + 2 samples behind P.  Every output is the fmaf chain of dcs_resample_f32 -- its phase row in ascending n from 0,
 * zero for inputs outside [0, L) -- so the concatenated outputs equal dcs_resample_f32 on the complete signal bit for bit,
 * however it is cut; they trail the input by half / up input samples.  State: one ring of max_push + 2 half / up + 2 samples
 * per row, allocated by create (1 <= max_push <= 2^30, else DCS_EINVAL); a push allocates nothing, reset reallocates nothing. */
typedef struct dcs_resample_stream dcs_resample_stream;
DCS_API int dcs_resample_stream_create(dcs_resampler* r, int rows, int64_t max_push, dcs_resample_stream** out);
DCS_API int dcs_resample_stream_destroy(dcs_resample_stream* s);
DCS_API int dcs_resample_stream_reset(dcs_resample_stream* s);
DCS_API int64_t dcs_resample_stream_bytes(const dcs_resample_stream* s);
/* Appends n samples per row (row k at in_d + k in_stride, 0 <= n <= max_push), last != 0 ends the signal, and writes the
 * outputs that became final (row k at out_d + k out_stride, *n_out of them per row, the formulas above).  DCS_EINVAL, before
 * anything is launched or written: n out of range, a push after the end, out_cap below what becomes final, strides below the
 * counts when rows > 1, a P up past int64.  Enqueued on the ctx stream of the plan. */
DCS_API int dcs_resample_stream_push(dcs_resample_stream* s, const float* in_d, int64_t in_stride, int64_t n, int last,
                                     float* out_d, int64_t out_stride, int64_t out_cap, int64_t* n_out);

/* ------------------------------------------------------------------ timing aid for bench.py */
/* Average duration (ms) of the kernels tagged `which` since the last reset, measured with HIP events
 * on the ctx stream.  tag_mask bit t enables the tag t (two event records per tagged launch);
 * 0 disables all. */
enum { DCS_TAG_STFT = 0, DCS_TAG_CONV1 = 1, DCS_TAG_CONV2 = 2, DCS_TAG_FC = 3, DCS_TAG_FC1X = 4,
       DCS_TAG_DECONV2 = 5, DCS_TAG_FINAL = 6, DCS_TAG_ISTFT = 7, DCS_TAG_OLA = 8, DCS_TAG_TILE = 9, DCS_TAG_POOL = 10,
       DCS_TAG_UNPOOL = 11, DCS_TAG_MASK = 12, DCS_TAG_SCORE = 13,
       DCS_TAG_DECODER = 14 /* transposed conv2 + transposed conv1 in one kernel (Bach10 graph, f16 switch) */,
       DCS_TAG_BSS_CORR = 15 /* dcs_bss_energies / dcs_bss_lagcorr: lag correlations, one bracket per window group */,
       DCS_TAG_BSS_CHOL = 16 /* dcs_bss_energies: Gram assembly, partial Cholesky, energies, one bracket per window group */,
       DCS_TAG_MWF = 17 /* dcs_mwf_f32: one bracket per pass */,
       DCS_TAG_COUNT = 18 };
DCS_API int dcs_timing_enable(dcs_ctx* ctx, unsigned tag_mask);
/* bracket only every stride-th launch of an enabled tag (an event pair costs ~6 us of stream time each side) */
DCS_API int dcs_timing_stride(dcs_ctx* ctx, int stride);
DCS_API int dcs_timing_reset(dcs_ctx* ctx);
DCS_API int dcs_timing_query(dcs_ctx* ctx, int which, double* avg_ms, int64_t* launches);

/* ------------------------------------------------------------------ training (csrc/train_core.hip; examples/dsd100/trainCNN.py:
 *                                                                     csrc/train_dsd.hip; examples/ikala/trainCNN.py: csrc/train_ikala.hip;
 *                                                                     examples/bach10/trainCNNbach10.py: csrc/train_bach10.hip; the
 *                                                                     last two on the shared build_ca graph csrc/train_ca.hip) */
/* The train_fn / train_fn1 pair of train_auto (trainCNN.py:132-263) for the DSD graph build_ca (:66-130; also what
 * examples/hiphopss/trainCNN.py trains): arch DCS_ARCH_DSD, time_context even in [4, 64], F <= 2049, batch 1 .. 1024, else
 * DCS_EINVAL; 15 arrays.  Or the pair of examples/ikala/trainCNN.py:120-197 for the iKala graph (:66-118): arch
 * DCS_ARCH_IKALA_NOPOOL, time_context 10 .. 64 (conv2 is 10 rows high), F 87 .. 2049 (conv2's output keeps a column),
 * batch 1 .. 1024, else DCS_EINVAL; 13 arrays.  Or the pair of examples/bach10/trainCNNbach10.py:126-206 for the Bach10 graph
 * (:66-123; trainCNNrwc.py and trainCNNSibelius.py train the same graph with the same loss): arch DCS_ARCH_BACH10,
 * time_context 2 .. 47 (conv2 is int(2 tc / 3) rows high; from 48 on dcs_model_create's bach10 graph has no column
 * convolution to run the result), F 30 .. 2049, batch 1 .. 1024, else DCS_EINVAL; 17 arrays.  The stereo, the score-informed
 * and the deep score-informed graphs are described below.  Any other arch (DCS_ARCH_IKALA, the pooled graph of
 * separate_ikala.py, included: the reference never trains it) is DCS_EUNSUPPORTED.  params_d / shapes / nparams as for dcs_model_create (.pkl
 * order), copied into the trainer.  rand_d [batch][1][tc][F]: the uniform draw baked into the loss (trainCNN.py:174), copied.
 * hyper_h: eps, alpha, beta, beta_voc (:169-172) -- for iKala eps, alpha, beta_acc, beta_voc (ikala/trainCNN.py:152-155); for
 * Bach10 eps (1e-18, bach10/trainCNNbach10.py:160) and three ignored values -- then adadelta's learning_rate, rho, epsilon (lasagne defaults 1, 0.95, 1e-6).  Adadelta's accu / delta_accu start at zero
 * (lasagne.updates.adadelta). */
DCS_API int dcs_trainer_create(dcs_ctx* ctx, int arch, int time_context, int F, int batch, const float* const* params_d,
                               const int64_t* shapes, int nparams, const float* rand_d, const double* hyper_h,
                               dcs_trainer** out);
DCS_API int dcs_trainer_destroy(dcs_trainer* t);
/* The score-informed Bach10 graph (examples/bach10_scoreinformed/trainCNNrwc.py: build_ca :134-193, train_fn / train_fn1
 * :225-283; csrc/train_bach10si.hip on csrc/train_ca.hip): dcs_trainer_create with arch DCS_ARCH_BACH10_SI (17 arrays) or DCS_ARCH_BACH10_SI1
 * (11 arrays, the single-branch form trainCNNrwc_samp.py:195-235 trains with the same loss, :275-321); time_context 2 .. 47
 * (the largest value for which dcs_model_create runs the score-informed graph: its inference kernels are the Bach10 graph's),
 * F 30 .. 2049, batch 1 .. 1024, else DCS_EINVAL.  rand_d [batch][1][tc][F]; hyper_h: eps (1e-18, :235), three ignored values,
 * adadelta's three.  dcs_trainer_step takes inputs_d [batch][4][tc][F] (the mixture times the four harmonic masks,
 * dcs_trainer_gather_score) and targets_d [batch][4][tc][F]; the loss reads prediction2[:, 0:4], the four channels of decoder
 * branch 0, against the mixture x = ((x0 + x1) + x2) + x3: masks p_k / (p_1 + .. + p_4 + eps r), the loss |error1 + .. +
 * error4|; out7 = (loss, error1 .. error4, 0, 0); the 0 / 0 NaN is kept.  dcs_trainer_forward writes p_d [batch][4][tc][F],
 * the live channels prediction2[:, 0:4].
 * Dead parameters: in the 17-array graph fc12, fc13, fc14 (arrays 10 .. 15) and bo[4:16] reach no loss term, so the
 * reference's gradient for them is exactly zero and Adadelta from a zero state never moves them or their accumulators.  The
 * trainer holds them once, outside the stepped state: dcs_trainer_get(which = 0) returns them bit-identical to what
 * dcs_trainer_create was given, which = 1, 2, 3 return zeros for them. */
/* The deep score-informed graph build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:66-132, --function build_ca_1x1;
 * csrc/train_deep1x1.hip): dcs_trainer_create with arch DCS_ARCH_BACH10_SI_1X1, 22 arrays in .pkl order: the whole graph
 * (the 1x1 layer [800][200][1][1], its two biases [800], the final bias [16]) or a live-only layout of k = 1 .. 3 branches
 * ([200 k][200][1][1], [200 k], [200 k], [4 k]).  time_context 19 .. 1024, F 253 .. 2049 (below 19 / 253 a convolution has no
 * output), batch 1 .. 1024, and 2 batch time_context ((F - 5) / 2 + 1) < 2^30: the K of conv1's weight gradient, the largest
 * index a GEMM of the step forms, stays in the 30 bits its index arithmetic has; anything else is DCS_EINVAL.  rand_d, hyper_h,
 * inputs_d, targets_d, out7, the loss (it reads prediction2[:, 0:4]: branch 0, rows 0 .. 199 of the 1x1 layer), the kept NaN
 * and dcs_trainer_forward are those of DCS_ARCH_BACH10_SI above.  Dead parameters: rows 200 .. of the 1x1 layer's W, b and
 * BiasLayer.b and the final bias from entry 4 on reach no loss term; they are held once outside the stepped state,
 * dcs_trainer_get(which = 0) returns them bit-identical to what create was given, which = 1, 2, 3 zeros.
 *
 * dcs_trainer_rectify_codes: r'(pre) of the seven rectified layers (conv1 .. conv6, the live 200 rows of the 1x1 layer) at the
 * last dcs_trainer_step / dcs_trainer_forward, as floats 0 / 0.5 / 1 (0.5: a pre-activation of exactly 0) into n = 7 device
 * buffers [batch][C_l][H_l][W_l].  These codes are what the step's gradient was computed with (the InverseLayers multiply
 * by them), so a float64 check of the gradient evaluates its graph at them.  DCS_EUNSUPPORTED for every other graph (they
 * keep pre-activations), DCS_ESHAPE for n != 7. */
DCS_API int dcs_trainer_rectify_codes(dcs_trainer* t, float* const* out_d, int n);
/* The stereo (ILD) DSD100 graph (examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py: build_ca :66-113, train_fn_mse / train_fn1
 * :183-206, train_fn_ILD :210-228 and :268; csrc/train_dsdild.hip): dcs_trainer_create with arch DCS_ARCH_DSD_ILD,
 * time_context even in [4, 64], F 1 .. 2049, batch 1 .. 1024, else DCS_EINVAL; 17 arrays.  rand_d [2][batch][4][tc][F]: the
 * two normal draws rand_num (:164) then rand_num2 (:210).  hyper_h: eps (1e-12, :152), ild_weight (1 / 500, :228), two
 * ignored values, then adadelta's three.  dcs_trainer_step takes inputs_d [batch][2][tc][F] and targets_d [batch][8][tc][F]
 * (channel 2 s + c: source s in input channel c); modes 0 / 1 / 2 use the stage-1 loss sum_j |sum (source_j - target_j)^2|
 * (:183-198), mode + 4 (4 / 5 / 6) the stage-2 loss, which adds ild_weight |sum_f (mean a_est[f] - mean a_gt[f])^2| with
 * a = 20 log10 |s_0 / (s_1 + eps r2) + eps r2| (:214-228); on any other graph mode + 4 is DCS_EINVAL.  The output vector
 * has 16 doubles: [0] the loss, [1 .. 8] errors_insts (:194: mic 0's four sources, then mic 1's), [9] the weighted ILD
 * term (0 in stage 1), [10 .. 15] zero.  Where all four outputs of a channel are zero and the draw is zero the
 * reference divides 0 by 0 (and takes log 0 where a level ratio is 0): the NaN / inf is kept.
 *
 * dcs_trainer_out_count: the doubles dcs_trainer_step writes for this trainer: 7, or 16 for DCS_ARCH_DSD_ILD. */
DCS_API int dcs_trainer_out_count(dcs_trainer* t, int* count);
/* Replace the draw, in stream order: rand_d has the size given at create ([batch][1][tc][F] for the mono graphs,
 * [2][batch][4][tc][F] for DCS_ARCH_DSD_ILD).  A difference from the reference worth knowing: there rand_num and rand_num2
 * of the stereo trainer come from RandomStreams(128).normal(std=0.1) and are REDRAWN on every call of a compiled function,
 * by Theano's MRG31k3p stream, which is not reproduced here; the trainer instead holds one draw until the caller replaces it
 * (examples/dsd100_2ch_ILD/train_dsd_ild.py does so before every step from a seeded device generator).  With eps = 1e-12
 * the draw only matters where a denominator would otherwise be zero; in silent target bins the ILD term depends on it. */
DCS_API int dcs_trainer_set_rand(dcs_trainer* t, const float* rand_d);
/* One step on inputs_d [batch][1][tc][F] and targets_d [batch][4][tc][F] (iKala: [batch][2][tc][F], voice then
 * accompaniment; Bach10: bassoon, clarinet, saxophone, violin) (trainCNN.py:243-263), no host synchronisation: mode 0 = train_fn1 (:263): forward, loss and components;
 * 1 also the gradients of |E|, one per parameter (Theano conventions: rectify'(0) = 0.5, abs'(0) = 0); 2 = train_fn (:262):
 * also the update: adadelta (:223) unless dcs_trainer_set_optimizer selected another.  out7_d (device, nullable): 7 doubles, all at the parameters BEFORE this step's update:
 * DSD the loss |E| then vocals, bass, drums, negative, alpha, negative_voc (:217, :263); iKala the loss |E| with E =
 * vocals_error + acc_error - negative_error_voc, then vocals_error, acc_error, negative_error_voc, negative_error_acc
 * (ikala/trainCNN.py:189, :197), then two zeros; Bach10 the loss |error1 + error2 + error3 + error4|, then the four errors
 * (bach10/trainCNNbach10.py:193-198, :206), then two zeros.  Bach10's masks are p_k / (p_1 + .. + p_4 + eps r): where all
 * four outputs are zero and r = 0 the reference divides 0 by 0, and the NaN is kept. */
DCS_API int dcs_trainer_step(dcs_trainer* t, const float* inputs_d, const float* targets_d, int mode, double* out7_d);
/* lasagne.layers.get_output(network2) (trainCNN.py:165) at the current parameters: p_d [batch][4][tc][F] (iKala
 * [batch][2][tc][F]), before masking */
DCS_API int dcs_trainer_forward(dcs_trainer* t, const float* inputs_d, float* p_d);
/* Copy one section of the trainer's state into 15 (iKala 13, Bach10 17, score-informed 17 or 11, deep score-informed 22) caller buffers in .pkl layout: which 0 = parameters
 * (get_all_param_values, trainCNN.py:59-64), 1 = the gradients of the last mode 1 / 2 step, 2 = adadelta accu,
 * 3 = adadelta delta_accu; under DCS_OPT_ADAM 2 = m, 3 = v. */
DCS_API int dcs_trainer_get(dcs_trainer* t, int which, float* const* out_d, int nparams);
/* The inverse of dcs_trainer_get, in stream order: lasagne.layers.set_all_param_values on the live network
 * (examples/bach10_scoreinformed/trainCNNrwc.py:349-351 reloads the best model before its second pass;
 * examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100_3stages.py:266-267 and :298-299 load a saved model between its stages) for
 * which = 0, and the same for the two accumulators of the selected update, which = 2 (adadelta accu, adam m) and 3 (adadelta
 * delta_accu, adam v).  in_d: nparams device arrays in .pkl order with the trainer's shapes, copied.  which = 1 (the
 * gradients, rewritten by every step) or anything else is DCS_EINVAL; a wrong nparams is DCS_ESHAPE ("mismatch: ...").
 * Nothing else changes: which = 0 keeps both accumulators and the step count.  Dead parameters (the score-informed graphs above)
 * are taken from which = 0 alone; for which = 2 and 3 their arrays are ignored and stay zero. */
DCS_API int dcs_trainer_set(dcs_trainer* t, int which, const float* const* in_d, int nparams);
/* Select the update that dcs_trainer_step mode 2 applies, which is what calling lasagne.updates.adadelta / lasagne.updates.adam
 * again does in the reference (trainCNNrwc.py:353 builds adam for the second pass; trainCNN_ILD_DSD100_3stages.py:269 rebuilds
 * adadelta for the ILD stage): kind DCS_OPT_ADADELTA with hyper_h = (learning_rate, rho, epsilon, unused; lasagne's defaults
 * 1, 0.95, 1e-6) or DCS_OPT_ADAM with hyper_h = (learning_rate, beta1, beta2, epsilon; 1e-3, 0.9, 0.999, 1e-8).  Both
 * accumulators (which = 2 and 3 of dcs_trainer_get) and the step count become zero, in stream order.  A trainer starts as
 * DCS_OPT_ADADELTA with hyper_h[4 .. 6] of dcs_trainer_create.  Adam is lasagne's: with t the step count after this step,
 * a_t = learning_rate sqrt(1 - beta2^t) / (1 - beta1^t) (computed on the host in double), m' = beta1 m + (1 - beta1) g,
 * v' = beta2 v + (1 - beta2) g^2, p' = p - a_t m' / (sqrt(v') + epsilon): epsilon outside the bias correction.  Where g, m
 * and v are zero the step is exactly zero.  DCS_EINVAL: an unknown kind, a learning rate that is negative or not finite,
 * rho or a beta outside [0, 1), epsilon <= 0 or not finite; the trainer is unchanged then. */
DCS_API int dcs_trainer_set_optimizer(dcs_trainer* t, int kind, const double* hyper_h);
/* The selected update: its kind, its four hyper-parameters as dcs_trainer_set_optimizer takes them, and the number of mode-2
 * steps since it was selected (Adam's t before the next step). */
DCS_API int dcs_trainer_get_optimizer(dcs_trainer* t, int* kind, double* hyper_h, int64_t* steps);
/* Set the step count (>= 0, else DCS_EINVAL): with dcs_trainer_set of both accumulators, the exact resume of a run (Adam's
 * a_t depends on it; lasagne/updates.py adam keeps t as a shared variable next to m and v). */
DCS_API int dcs_trainer_set_steps(dcs_trainer* t, int64_t steps);
/* LargeDataset's windows (dataset.py:383-488) from feature files resident on the device: data_d holds every file's
 * [5][T_i][F] float32 block (mixture, vocals, bass, drums, other), files_d [n_files][2] int64 = (element offset, T_i),
 * windows_d [batch][2] int32 = (file, first frame); file < 0 is an all-zero window (initOutput, :509-516), frames past T_i are
 * zero (the padded window of a file shorter than tc, :431-437).  inputs_d [batch][1][tc][F] = scale * mixture,
 * targets_d [batch][4][tc][F] = scale * sources (mult_factor_in / _out, :421-428). */
DCS_API int dcs_trainer_gather(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d, int batch,
                               int time_context, int F, float scale, float* inputs_d, float* targets_d);
/* dcs_trainer_gather for feature files of nsrc sources (1 .. 8): data_d holds [1 + nsrc][T_i][F] blocks (mixture, then
 * the sources; iKala: mixture, voice, accompaniment, examples/ikala/compute_features.py), targets_d [batch][nsrc][tc][F]. */
DCS_API int dcs_trainer_gather_sources(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d,
                                       int batch, int time_context, int F, int nsrc, float scale, float* inputs_d,
                                       float* targets_d);
/* LargeDatasetMulti's windows (dataset.py:921-1007): data_d holds per file one [cin + cout][T_i][F] block, the `in` tensor's
 * channels (*_in_m_.data) first, then the `out` tensor's (*_out_m_.data); cin 1 .. 4, cout 1 .. 16.  The window table and the
 * zero / padding rules are dcs_trainer_gather's.  inputs_d [batch][cin][tc][F] = scale_in * in, targets_d
 * [batch][cout][tc][F] = scale_out * out (mult_factor_in / mult_factor_out). */
DCS_API int dcs_trainer_gather_channels(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d,
                                        int batch, int time_context, int F, int cin, int cout, float scale_in,
                                        float scale_out, float* inputs_d, float* targets_d);
/* The score-informed feed (dataset.py LargeDatasetMask2: loadFile :383-488 with filterSpec :839-879, then
 * trainCNNrwc.py:309-320), one launch per batch from data resident on the device.  data_d / files_d / windows_d as for
 * dcs_trainer_gather_sources with nsrc = ninst: per file a [1 + ninst][T_i][F] block (Bach10: mixture, bassoon, clarinet,
 * saxophone, violin).  notes_d: every file's packed note table (dcs_trainer_pack_score), note_files_d [n_files][2] int64 =
 * (offset in ints, notes per instrument).  targets_d [batch][ninst][tc][F] = scale * source_j; inputs_d [batch][ninst][tc][F]
 * = mask_j * (scale * mixture) with mask_j = filtered_j / sum_i filtered_i in float32, the instruments added in order,
 * filtered = 1 on the note rectangles and 1e-18 elsewhere: the rectangle rule of dcs_score_masks_norm(.., start, start + tc,
 * DCS_SCORE_NORM_SUM, ..).  Every product is rounded once to float32.  Zero slots (file < 0) and frames past T_i are zero in
 * both outputs.  ninst 1 .. 32, width = 2 nharmonics + 3 (odd, from 5), else DCS_EINVAL.  The timbre-model branch of
 * filterSpec is not part of the feed. */
DCS_API int dcs_trainer_gather_score(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* notes_d,
                                     const int64_t* note_files_d, const int* windows_d, int batch, int time_context, int F,
                                     int ninst, int width, float scale, float* inputs_d, float* targets_d);
/* The feed of the augmented trainers (examples/hiphopss/augmentations/trainCNN_{cs,instr,mix}_aug.py), in place of the
 * compute_features_*_aug.py files read back by LargeDataset (dataset.py:383-488): the windows are transformed from source
 * audio resident on the device, rendered by the rule of dcs_stft_forward_render.  bank_d [bank_len] float32.  files_d
 * [n_files][DCS_RENDER_ROW(S)] int64: per virtual file -- what one .data file of the reference holds, i.e. one chunk of one
 * variant -- (size, a, Lc, T = dcs_frame_count(Lc, hop)) then (offset, L_s, k_s, c_s) per track; gains_d [n_files][1 + S]
 * float64 = (m, g_s).  windows_d [batch][2] int32 = (virtual file, first frame) with dcs_trainer_gather's zero rules: file
 * < 0 (or >= n_files) is an all-zero window, frames past T are zero.  inputs_d [batch][1][tc][F] = scale * mag(mix),
 * targets_d [batch][S][tc][F] = scale * mag(r_s) at channel c_s - 1, F = frame / 2 + 1; each product rounded once to
 * float32.  One launch per batch, no intermediate audio or feature buffer.  The table lives on the device, so the kernel
 * bounds it: samples outside the bank read as zero, a channel outside 1 .. S is not written.  S 1 .. 8, batch and
 * time_context >= 1, else DCS_EINVAL. */
DCS_API int dcs_trainer_gather_render(dcs_ctx* ctx, dcs_stft* plan, const float* bank_d, int64_t bank_len,
                                      const int64_t* files_d, const double* gains_d, int n_files, const int* windows_d,
                                      int batch, int time_context, int S, float scale, float* inputs_d, float* targets_d);
/* The feed of the Bach10 trainers on RWC-sample data (examples/bach10/trainCNNrwc.py), in place of the
 * compute_features_bach10rwc.py files (:112-141, one float64 file per combination and score chunk) read back by
 * LargeDataset (dataset.py:383-488): the windows are transformed from a bank of note samples resident on the device, by the
 * rule of dcs_stft_forward_score_render.  bank_d [bank_len] float32.  notes_d [n_notes][4] int64 as dcs_score_render_pack
 * wrote it; files_d [n_files][DCS_SCORE_RENDER_ROW(S)] int64: per virtual file (size, T = dcs_frame_count(size, hop)) then
 * (first note, note count) per track.  windows_d [batch][2] int32 = (virtual file, first frame) with dcs_trainer_gather's
 * zero rules: file < 0 or >= n_files and frames past T give zero rows.  inputs_d [batch][1][tc][F] = scale * mag(mix),
 * targets_d [batch][S][tc][F] = scale * mag(track_s), F = frame / 2 + 1, each product rounded once to float32.  One launch
 * per batch.  The tables live on the device, so the kernel bounds them: a track whose notes lie outside the table is
 * silent, samples outside the bank read as zero.  S 1 .. 8, batch, time_context, n_files and bank_len >= 1, else
 * DCS_EINVAL. */
DCS_API int dcs_trainer_gather_score_render(dcs_ctx* ctx, dcs_stft* plan, const float* bank_d, int64_t bank_len,
                                            const int64_t* notes_d, int64_t n_notes, const int64_t* files_d, int n_files,
                                            const int* windows_d, int batch, int time_context, int S, float scale,
                                            float* inputs_d, float* targets_d);
/* The feed of the score-informed Bach10 trainer on RWC-sample data (examples/bach10_scoreinformed/trainCNNrwc.py), in place
 * of the compute_features_bach10rwc.py files (:96-163: per combination and score chunk a float64 [5][T][F] block and two note
 * tables) read back by LargeDatasetMask2: dcs_trainer_gather_score_render and dcs_trainer_gather_score in one launch per
 * batch, with no intermediate audio or feature buffer.  ctx .. n_files, windows_d .. scale as for
 * dcs_trainer_gather_score_render.  masks_d [mask_len] int32: every virtual file's mask table [S][P][width - 1] exactly as
 * dcs_trainer_pack_score writes it (ninst = S); mask_files_d [n_files][2] int64 = (offset in ints, P); width = 2 nharmonics
 * + 3.  targets_d [batch][S][tc][F] = scale * mag(track_s); inputs_d [batch][S][tc][F] = mask_j * (scale * mag(mix)), the
 * arithmetic of dcs_trainer_gather_score operation for operation: filtered = 1 on the rectangles (a note paints frame fr of
 * the virtual file when first <= fr < end) and 1e-18 elsewhere, the instruments added in order in float32, one division,
 * one product.  Both outputs equal, bit for bit, dcs_trainer_gather_score on the blocks dcs_stft_forward_score_render_f32
 * writes.  Zero rows (both outputs): file < 0, file >= n_files, frames past T.  The tables live on the device, so the
 * kernel bounds them: a mask table that does not lie inside [0, mask_len) paints nothing (every mask is 1 / S up to the
 * float32 sum), bins are clipped to [0, F), a track whose render notes lie outside the note table is silent, samples
 * outside the bank read as zero.  DCS_EINVAL, launching nothing: a null argument, a plan of another context, S outside 1 ..
 * 8, width even or below 5 (a packed note is 2 npairs + 2 = width - 1 ints), batch, time_context, n_files or bank_len
 * below 1, mask_len or n_notes negative. */
DCS_API int dcs_trainer_gather_score_informed_render(dcs_ctx* ctx, dcs_stft* plan, const float* bank_d, int64_t bank_len,
                                                     const int64_t* notes_d, int64_t n_notes, const int64_t* files_d,
                                                     int n_files, const int* masks_d, int64_t mask_len,
                                                     const int64_t* mask_files_d, int width, const int* windows_d, int batch,
                                                     int time_context, int S, float scale, float* inputs_d, float* targets_d);
/* One file's note table notes_h [ninst][n_notes][width] (first frame, end frame, MIDI number, then width - 3 values: first
 * bin, end bin per harmonic; util.expandMidi) -> packed_h [ninst][n_notes][width - 1] ints for dcs_trainer_gather_score, on
 * the host.  Notes with MIDI number <= 0 and bands with end bin <= 0 are dropped, as filterSpec drops them.  A band outside
 * [0, F) is DCS_ESHAPE (the reference's bin index would raise for every window that holds the note). */
DCS_API int dcs_trainer_pack_score(const double* notes_h, int ninst, int n_notes, int width, int F, int* packed_h);

/* ------------------------------------------------------------------ memory-safety aid (tests/test_gpu_guard.py) */
/* With DCS_WS_GUARD=<bytes> in the environment (read once per process) every scratch block libdcs allocates -- the
 * per-model workspace, the K-split partial sums, the clip / note tables -- sits between two red zones of that size and is
 * born filled with the byte DCS_WS_POISON (default 0xFF: float NaN).  This call synchronises the device and verifies every
 * live red zone: DCS_OK, DCS_EHIP with the first damaged byte in dcs_last_error(), DCS_EUNSUPPORTED without the switch.
 * No reference counterpart (the reference is NumPy / Theano); n_blocks_out (nullable) = guarded blocks alive. */
DCS_API int dcs_debug_check_guards(dcs_ctx* ctx, int64_t* n_blocks_out);

/* Test aids for the transform kernels (tests/test_gpu_stft_kernels.py); no reference counterpart.  The two launchers below
 * are the ones dcs_separate* use internally -- the forward one writes unit phasors X / |X| ((1, 0) where X == 0) next to the
 * magnitudes, the inverse one reads them instead of an angle -- reached here with every argument checked first: DCS_EINVAL
 * and no launch for a null pointer, a negative count, ld < frame / 2 + 1, a stride shorter than what it strides over, or a
 * clip table that points outside the buffers as these arguments describe them.  The table is on the device and is read back
 * (one stream synchronisation per call: these are no production entry points).
 *
 * forward: n_clips signals of n_samples each, signal c at audio_d + c * audio_stride.  T = dcs_frame_count(n_samples, hop);
 * mag_d / phase_d (nullable) / unit_d (nullable, (re, im) pairs) hold n_clips * rows_out rows of ld values, rows_out >= T,
 * clip c at row c * rows_out -- or, with interleave != 0, row t * n_clips + c.  Rows past a clip's frames and columns past
 * frame / 2 are written as magnitude 0, phase 0, phasor (1, 0).  clip_tab_d (nullable; frameSize 1024 / 2048 / 4096 only,
 * else DCS_EUNSUPPORTED; not with interleave): per clip six int64 {samples, frames, tiles, row offset, tile offset, rows}
 * with samples <= n_samples and frames = dcs_frame_count(samples, hop) <= rows_out.  Row offset < 0 in every clip: the
 * pitch above applies.  Otherwise in every clip: clip c owns rows [row offset, row offset + rows) of the buffers, frames <=
 * rows <= rows_out, inside the n_clips * rows_out rows. */
DCS_API int dcs_debug_stft_forward_f32(dcs_stft* plan, const float* audio_d, int64_t n_samples, int64_t audio_stride,
                                       int64_t n_clips, float* mag_d, float* phase_d, float* unit_d, int64_t ld,
                                       int64_t rows_out, int interleave, const int64_t* clip_tab_d);
/* inverse: n_clips clips of n_src sources each.  Source s of clip c reads the magnitudes at mag_d + (c * n_src + s) *
 * src_stride ([n_frames, ld]) and the clip's phasors at unit_d + c * unit_clip_stride ([n_frames, ld] pairs), and writes
 * n_out <= dcs_inverse_length(n_frames, hop, frame) samples at audio_d + (c * n_src + s) * out_stride (out_stride 0: n_out;
 * samples [n_out, out_stride) are not written).  X = (mag / pre_div) * sqrt(frame) * unit; imaginary parts at bins 0 and
 * frame / 2 are ignored.  clip_tab_d (nullable; needs frameSize 1024 / 2048 / 4096 and an even hop that divides it, else
 * DCS_EUNSUPPORTED): clip c has samples <= n_out samples and frames <= n_frames frames; with row offsets >= 0 its phasor
 * rows start at row `row offset` of unit_d instead and must end inside the rows the strides describe. */
DCS_API int dcs_debug_stft_inverse_unit_f32(dcs_stft* plan, const float* mag_d, int64_t src_stride, const float* unit_d,
                                            int64_t unit_clip_stride, int64_t ld, int64_t n_frames, int n_src,
                                            int64_t n_clips, float pre_div, float* audio_d, int64_t n_out,
                                            const int64_t* clip_tab_d, int64_t out_stride);
/* Which kernel the plan's last forward / last inverse launch ran (any entry point, dcs_separate* included; 0 = none yet),
 * and in *param the number of hop-blocks per workgroup (block, ring), per wave (seq) or of frames per wave (chain) that the
 * inverse launcher chose.  Host-side bookkeeping, one store per launch.  Every pointer is nullable. */
#define DCS_STFT_FWD_BLOCK 1      /* one workgroup per frame (any frameSize, float64) */
#define DCS_STFT_FWD_WAVE1 2      /* one wave per frame, one frame per workgroup */
#define DCS_STFT_FWD_WAVE4 3      /* one wave per frame, four frames per workgroup */
#define DCS_STFT_INV_BLOCK 1      /* accumulator in LDS, one workgroup per run of hops (any size, float64) */
#define DCS_STFT_INV_RING 2       /* four waves, ring of hop-blocks in LDS */
#define DCS_STFT_INV_SEQ 3        /* one wave per run of hop-blocks, blocks in registers */
#define DCS_STFT_INV_SEQ_STAGED 4 /* the same with the spectra brought in through LDS */
#define DCS_STFT_INV_CHAIN 5      /* eight waves walk consecutive runs of frames and meet at seams */
DCS_API int dcs_debug_stft_last_kernel(const dcs_stft* plan, int* forward, int* inverse, int64_t* param);

/* Test aids for the GEMM kernels and operand packers of csrc/gemm.hip, gemm_bf16x3.hip and gemm_f16.hip
 * (tests/test_gpu_gemm_kernels.py); no reference counterpart.  The contract of every kernel:
 *   C[crow(r)][0 .. n_store) = act(a_scale * A[arow(r)][0 .. K) . B[K][ldb] + bias),   r = 0 .. M - 1
 *   arow(r) = a_rowmap ? a_rowmap[r] : (r / a_gdiv) * a_gmul + r % a_gdiv  (rows of lda floats), crow alike with ldc.
 * B is padded with zero rows to round_up(K, 128) rows, ldb and n_cols are multiples of 64.  Every buffer comes with its
 * element count (n_*: floats, ints for the row map; *_bytes: bytes) and the entry refuses with DCS_EINVAL, launching
 * nothing, an argument set whose largest address lies outside those counts -- the row map is read back from the device
 * and checked (one stream synchronisation per call: these are no production entry points) -- or whose pointers are not
 * 16-byte aligned.  A launcher that does not take the shape yields DCS_EUNSUPPORTED.
 *   which = DCS_GEMM_VIA_ROWS   dcs_launch_gemm_rows, the launcher of the graphs, with its own choice of kernel and its
 *                               own refusals (n_cols % 64; a_vec with K % 4 or lda % 4)
 *           DCS_GEMM_VIA_SKINNY the all-rows bf16 x 3 kernel; n_br = 0: Bq / bias / C, n_br = 1 .. 4: br_Bq / br_bias /
 *                               br_C (each of Bq_bytes, n_bias, n_C; a branch's bias may be null)
 *           DCS_GEMM_VIA_LONGK  the bf16 x 3 long-K launch (slices into the context's scratch, then the reduce pass)
 * Bq (nullable): dcs_debug_gemm_pack's DCS_GEMM_PACK_BQ planes, or with bq_f32 its DCS_GEMM_PACK_B32 pieces; Aq
 * (nullable): DCS_GEMM_PACK_SPLIT_A planes of aq_rows rows; Bfrag (nullable): DCS_GEMM_PACK_BFRAG order. */
typedef struct dcs_debug_gemm_args {
    const float* A; int64_t n_A; int64_t lda; int32_t a_gdiv; int64_t a_gmul; float a_scale;
    const int32_t* a_rowmap; int64_t n_rowmap;
    const float* B; int64_t n_B; int32_t ldb;
    const float* bias; int64_t n_bias;
    float* C; int64_t n_C; int64_t ldc; int32_t c_gdiv; int64_t c_gmul;
    int64_t M; int32_t n_cols, n_store, K, relu, a_vec;
    const void* Bq; int64_t Bq_bytes; int32_t bq_f32;
    const void* Aq; int64_t Aq_bytes; int32_t aq_rows;
    const float* Bfrag; int64_t n_Bfrag;
    int32_t n_br;
    const void* br_Bq[4]; const float* br_bias[4]; float* br_C[4];
} dcs_debug_gemm_args;
#define DCS_GEMM_VIA_ROWS 0
#define DCS_GEMM_VIA_SKINNY 1
#define DCS_GEMM_VIA_LONGK 2
DCS_API int dcs_debug_gemm(dcs_ctx* ctx, int which, const dcs_debug_gemm_args* args);
/* The f16 all-rows kernel: C_b[M][n_cols] halves (ldc apart) = f16(relu(Z . Bh_b + bias_b)), b < n_br; Z [M][K] floats ldz
 * apart; Bh_b: DCS_GEMM_PACK_BH planes of Bh_bytes each; bias_b: n_bias >= n_cols floats; C_b: n_C halves; Ah_scratch:
 * Ah_bytes >= dcs_debug_gemm_bytes(DCS_GEMM_PACK_SPLIT_A_F16, K, M <= 128 ? 128 : 176) -- the launcher leaves A's two f16
 * planes there ([k tile][plane][rows][4 pieces of 8 k]; rows >= M zero). */
DCS_API int dcs_debug_gemm_f16_skinny(dcs_ctx* ctx, const float* Z_d, int64_t n_Z, int64_t ldz, int M, int K, int n_cols,
                                      int n_br, const void* const* Bh_d, int64_t Bh_bytes, const float* const* bias_d,
                                      int64_t n_bias, void* const* C_d, int64_t n_C, int64_t ldc, void* Ah_scratch_d,
                                      int64_t Ah_bytes);
/* The f16 long-K kernel and the reduce pass behind it: C[M][n_store) floats = act(A . Bh + bias).  A: n_A elements, floats
 * (a_f16 = 0) or halves (a_f16 != 0: K == lda, lda % 32 == 0); Bh: one f16 plane of n_cols columns. */
DCS_API int dcs_debug_gemm_f16_longk(dcs_ctx* ctx, const void* A_d, int64_t n_A, int64_t lda, int M, int K, int n_cols,
                                     const void* Bh_d, int64_t Bh_bytes, int a_f16, const float* bias_d, int64_t n_bias,
                                     float* C_d, int64_t n_C, int64_t ldc, int n_store, int relu);
/* The packing kernels.  p[0 .. 3] by kind:
 *   DCS_GEMM_PACK_BQ / _B32     src B [K][ld] floats, n columns; p = {perm_c, perm_p}: output column j < perm_c * perm_p is
 *                               source column (j % perm_c) * perm_p + j / perm_c
 *   DCS_GEMM_PACK_BH            src B [K][ld], n output columns; p = {nch, npos, chpad}: output column pos * chpad + ch is
 *                               source column ch * npos + pos, zero for ch >= nch or pos >= npos.  _BH_PLAIN: no p
 *   DCS_GEMM_PACK_BIAS_CL       src bias [nch * npos], n outputs, p as for _BH; K and ld unused
 *   DCS_GEMM_PACK_SPLIT_A       src A [p[0] = M rows][ld], n = rows_pad
 *   DCS_GEMM_PACK_BFRAG         on the HOST: src and dst are host pointers (the packer of the DSD model's folded layer)
 * dst holds dst_bytes >= dcs_debug_gemm_bytes(kind, K, n) bytes.  DCS_GEMM_PACK_SPLIT_A_F16 has a size only: its kernel
 * runs inside dcs_debug_gemm_f16_skinny. */
#define DCS_GEMM_PACK_BQ 0
#define DCS_GEMM_PACK_B32 1
#define DCS_GEMM_PACK_BH 2
#define DCS_GEMM_PACK_BH_PLAIN 3
#define DCS_GEMM_PACK_BIAS_CL 4
#define DCS_GEMM_PACK_SPLIT_A 5
#define DCS_GEMM_PACK_BFRAG 6
#define DCS_GEMM_PACK_SPLIT_A_F16 7
DCS_API int64_t dcs_debug_gemm_bytes(int kind, int K, int n);
DCS_API int dcs_debug_gemm_pack(dcs_ctx* ctx, int kind, const float* src, int64_t n_src, int K, int64_t ld, int n,
                                const int64_t* p, void* dst, int64_t dst_bytes);
/* Which kernel the context's last GEMM launch ran (any entry point; 0 = none yet) and params = {K slices, K per slice, row
 * blocks of 16 per workgroup, 1 if pre-split rows (Aq) were used}, 0 where there is none.  One host store per launch. */
#define DCS_GEMM_K_ROWS_1_128 1          /* gemm_rows_kernel<1, 128, false>; + 1: the float4 (a_vec) instance */
#define DCS_GEMM_K_ROWS_1_128_VEC 2
#define DCS_GEMM_K_ROWS_1_32 3
#define DCS_GEMM_K_ROWS_1_32_VEC 4
#define DCS_GEMM_K_ROWS_2_32 5
#define DCS_GEMM_K_ROWS_2_32_VEC 6
#define DCS_GEMM_K_ROWS_4_32 7
#define DCS_GEMM_K_ROWS_4_32_VEC 8
#define DCS_GEMM_K_SPLITK 9              /* gemm_rows_splitk_kernel<false>, all of K */
#define DCS_GEMM_K_SPLITK_BFRAG 10       /* gemm_rows_splitk_kernel<true> */
#define DCS_GEMM_K_KSPLIT_16 11          /* gemm_rows_splitk_kernel<false> per K slice + gemm_ksplit_reduce_kernel */
#define DCS_GEMM_K_KSPLIT_64 12          /* gemm_rows_kernel<4, 32, true> per K slice + gemm_ksplit_reduce_kernel */
#define DCS_GEMM_K_BF16X3_2 13           /* gemm_bf16x3_kernel<2> */
#define DCS_GEMM_K_BF16X3_4 14
#define DCS_GEMM_K_SKINNY_8 15           /* gemm_bf16x3_skinny_kernel<8, 2>; + 1: AQ, + 2: B32 */
#define DCS_GEMM_K_SKINNY_8_AQ 16
#define DCS_GEMM_K_SKINNY_8_B32 17
#define DCS_GEMM_K_SKINNY_8_AQ_B32 18
#define DCS_GEMM_K_SKINNY_11 19
#define DCS_GEMM_K_SKINNY_11_AQ 20
#define DCS_GEMM_K_SKINNY_11_B32 21
#define DCS_GEMM_K_SKINNY_11_AQ_B32 22
#define DCS_GEMM_K_LONGK_8 23            /* the same kernel per K slice + gemm_longk_reduce_kernel; + 1: B32 */
#define DCS_GEMM_K_LONGK_8_B32 24
#define DCS_GEMM_K_LONGK_11 25
#define DCS_GEMM_K_LONGK_11_B32 26
#define DCS_GEMM_K_F16_SKINNY_8 27       /* gemm_split_a_f16_kernel + gemm_f16_skinny_kernel<8> */
#define DCS_GEMM_K_F16_SKINNY_11 28
#define DCS_GEMM_K_F16_LONGK_8 29        /* gemm_f16_longk_kernel<8, false>; + 1: f16 rows (A16) */
#define DCS_GEMM_K_F16_LONGK_8_A16 30
#define DCS_GEMM_K_F16_LONGK_11 31
#define DCS_GEMM_K_F16_LONGK_11_A16 32
DCS_API int dcs_debug_gemm_last_kernel(const dcs_ctx* ctx, int* code, int64_t* params);

/* Test aids for the convolution kernels of the generic graphs (ikala / bach10 / score-informed: csrc/generic.hip,
 * slabconv_ps.hip, colconv_fwd_x3.hip, colconv_wreg.hip, colconv_x3.hip, conv1_mfma.hip, deconv1_mfma.hip;
 * tests/test_gpu_conv_kernels.py); no reference counterpart.  dcs_debug_conv_stage runs ONE stage of a model's forward
 * pass -- the very function the graph calls, so the choice of kernel is the production one -- on the caller's buffers:
 *   DCS_CONV_STAGE_CONV1    tiles [n][C][tc][F] -> a1b (and, in a graph with a pool layer, p1)
 *   DCS_CONV_STAGE_CONV2    a1b (p1 in a graph with a pool layer), laid out as a1_layout / a1_rows say -> a2b
 *   DCS_CONV_STAGE_DECODER  D, laid out as d_layout says -> o [n][n_branch * C][tc][F] (through g2, g1 where the two
 *                           InverseLayers run as separate kernels; a graph with a pool layer reads a1b as conv1 left it)
 * Every buffer a stage can touch comes with its byte count and must be 16-byte aligned and hold what the forward pass
 * itself would have carved for n tiles and n_branch branches:
 *   tiles n C tc F floats | a1b n nf1 tc w1 floats | p1 n nf1 tc wp | a2b n flat_p | D n n_branch flat_p (f16 layout: n
 *   n_branch round_up(32 h2 w2, 128) halves if that is more) | g2 n n_branch nf1 tc wp | g1 n n_branch nf1 tc w1 | o n n_branch C tc F
 * (flat_p = nf2 h2 w2 rounded up to 4).  DCS_EINVAL, and nothing launched, for a null or misaligned buffer the stage needs, a
 * short byte count, n or n_branch out of range, an unknown layout or tie mode.  DCS_EUNSUPPORTED, and nothing launched, for a
 * layout the model's plan cannot consume (a channels-last a1 without the kernel that reads it; a channels-last D where
 * the decoder would not run as one kernel and would have to redo the dense layers, which needs their input).
 * conv1 may be given the clip's frames (frames_src [C][frames_rows][F], tile k = rows k * frames_stride .. + tc, frames_rows =
 * (n - 1) * frames_stride + tc, 0 < frames_stride < tc): it then runs per frame where the graph would.  On return a1_layout,
 * a1_rows, fold2 and a2_f16 hold what the stage handed on (conv2 reads the first two as its input).  One stream
 * synchronisation per call.  The model is left as it was found, except that conv2 may pack the f16 plane of the bottleneck
 * weights on first need, as a forward pass of the same size would. */
#define DCS_CONV_STAGE_CONV1 0
#define DCS_CONV_STAGE_CONV2 1
#define DCS_CONV_STAGE_DECODER 2
#define DCS_CONV_LAYOUT_CHANNEL_FIRST 0   /* f32 [image][channel][row][x] */
#define DCS_CONV_LAYOUT_CL_F32 1          /* f32 [image][row][x][channel] */
#define DCS_CONV_LAYOUT_CL_F16 2          /* f16 [image][row][x][32], channels 30 and 31 zero */
typedef struct dcs_debug_conv_args {
    int64_t n; int32_t n_branch, tie_mode;
    const float* tiles; int64_t tiles_bytes;
    void* a1b; int64_t a1b_bytes;
    void* p1; int64_t p1_bytes;
    void* a2b; int64_t a2b_bytes;
    void* D; int64_t D_bytes;
    void* g2; int64_t g2_bytes;
    void* g1; int64_t g1_bytes;
    void* o; int64_t o_bytes;
    const float* frames_src; int64_t frames_bytes; int32_t frames_rows, frames_stride;
    int32_t a1_layout, a1_rows;           /* in: conv2; out: conv1 */
    int32_t d_layout;                     /* in: decoder */
    int32_t fold2, a2_f16;                /* out: conv2 */
} dcs_debug_conv_args;
DCS_API int dcs_debug_conv_stage(dcs_model* m, int stage, dcs_debug_conv_args* args);
/* Which kernel each role of the model's context launched last (any entry point; 0 = none since the last
 * dcs_debug_conv_stage began, which clears them) and three choices of its launcher: codes[DCS_CONV_ROLES],
 * params[DCS_CONV_ROLES][3] = {band, column tile, tap pairs per weight stage} for the slab kernels, else {column blocks per
 * workgroup, runs per image, workgroups} (0 where there is none).  Host-side bookkeeping, one store per launch. */
#define DCS_CONV_ROLE_CONV1 0
#define DCS_CONV_ROLE_POOL 1
#define DCS_CONV_ROLE_CONV2 2
#define DCS_CONV_ROLE_CONV2T 3
#define DCS_CONV_ROLE_UNPOOL 4
#define DCS_CONV_ROLE_CONV1T 5
#define DCS_CONV_ROLE_DECODER 6           /* both InverseLayers as one kernel */
#define DCS_CONV_ROLE_PAD 7               /* zero_pad_cols_kernel in front of conv2 */
#define DCS_CONV_ROLES 8
#define DCS_CONV_K_CONV1 1                /* conv1_kernel<30> */
#define DCS_CONV_K_CONV1_REG4 2           /* conv1_reg_kernel<30, 4> */
#define DCS_CONV_K_CONV1_REG3 3           /* conv1_reg_kernel<30, 3> */
#define DCS_CONV_K_CONV1_REG3_POOL 4      /* conv1_reg_kernel<30, 3, true> */
#define DCS_CONV_K_CONV1_MFMA_1 5         /* conv1_mfma_kernel<1, 0>; + 1: channels-last, + 2: f16 channels-last */
#define DCS_CONV_K_CONV1_MFMA_1_CL 6
#define DCS_CONV_K_CONV1_MFMA_1_CL16 7
#define DCS_CONV_K_CONV1_MFMA_4 8         /* conv1_mfma_kernel<4, 0>; + 1: channels-last */
#define DCS_CONV_K_CONV1_MFMA_4_CL 9
#define DCS_CONV_K_POOL 10                /* pool_kernel */
#define DCS_CONV_K_UNPOOL 11              /* unpool_kernel<4> */
#define DCS_CONV_K_IGEMM 12               /* conv_igemm_kernel, forward */
#define DCS_CONV_K_IGEMM_T 13             /* conv_igemm_kernel, transposed */
#define DCS_CONV_K_IGEMM_F16 14           /* conv_igemm_f16_kernel (either direction: the role says which) */
#define DCS_CONV_K_SLAB_MX_0 15           /* slabconv_mx_kernel<0>; + 1: <1> */
#define DCS_CONV_K_SLAB_MX_1 16
#define DCS_CONV_K_SLAB_PS_0 17           /* slabconv_ps_kernel<0, 16, false, true>, row bands; + 1: mode 1 */
#define DCS_CONV_K_SLAB_PS_1 18
#define DCS_CONV_K_SLAB_PS_STRIP_0 19     /* the same kernel on column strips; + 1: mode 1 */
#define DCS_CONV_K_SLAB_PS_STRIP_1 20
#define DCS_CONV_K_SLAB_PS_COL_0 21       /* slabconv_ps_kernel<0, 16, true, false>: kw == 1 */
#define DCS_CONV_K_COLCONV 22             /* colconv_kernel, forward */
#define DCS_CONV_K_COLCONV_T 23           /* colconv_kernel, transposed */
#define DCS_CONV_K_COLCONV_F16 24         /* colconv_f16_kernel (either direction) */
#define DCS_CONV_K_COLCONV_FWD_X3 25      /* colconv_fwd_x3_kernel<20, 30> */
#define DCS_CONV_K_WREG_SCATTER 26        /* colconv_wreg_scatter_kernel<20, 30, 8, false, false>; + 1: f16 in, + 2: f16 out */
#define DCS_CONV_K_WREG_SCATTER_I16 27
#define DCS_CONV_K_WREG_SCATTER_O16 28
#define DCS_CONV_K_WREG_SCATTER_I16_O16 29
#define DCS_CONV_K_WREG_GATHER 30         /* colconv_wreg_gather_kernel<20, 11> */
#define DCS_CONV_K_DECONV1 31             /* deconv1_kernel<30> */
#define DCS_CONV_K_DECONV1_REG3 32        /* deconv1_reg_kernel<3, 10> */
#define DCS_CONV_K_DECONV1_REG3_POOL 33   /* deconv1_reg_kernel<3, 10, true> */
#define DCS_CONV_K_DECONV1_REG4 34        /* deconv1_reg_kernel<4, 8> */
#define DCS_CONV_K_DECONV1_MFMA_1 35      /* deconv1_mfma_kernel<1> */
#define DCS_CONV_K_DECONV1_MFMA_4 36      /* deconv1_mfma_kernel<4> */
#define DCS_CONV_K_FUSED 37               /* colconv_deconv1_fused_kernel<20, 11, false, false>; + 1: channels-last, + 2: f16 */
#define DCS_CONV_K_FUSED_CL 38
#define DCS_CONV_K_FUSED_CL16 39
#define DCS_CONV_K_FUSED_X3_1 40          /* colconv_deconv1_fused_x3_kernel<20, 11, 1> */
#define DCS_CONV_K_FUSED_X3_4 41          /* colconv_deconv1_fused_x3_kernel<20, 11, 4> */
#define DCS_CONV_K_ZERO_PAD 42            /* zero_pad_cols_kernel */
#define DCS_CONV_K_UNLISTED 255           /* an instance no graph reaches today (slabconv_ps_kernel without its tap-pair mask, or kw == 1 on one f16 plane) */
DCS_API int dcs_debug_conv_last_kernel(const dcs_model* m, int* codes, int64_t* params);
/* The weights of conv2 + BiasLayer + bottleneck layer folded into one affine map of conv2's input (fold_conv2_fc_kernel),
 * copied to out_h (HOST memory, n_out floats of room): [rows = nf1 * tc * wp, row (ci, r, x)][cols = the hidden width rounded
 * up to 64]; *rows and *cols (nullable) are set, and with out_h null only they.  A model that runs folded (the iKala graphs
 * where conv2 costs at least four times what the fold adds to the layer, e.g. 513 bins) hands out the weights it uses; for a
 * smaller one the kernel is run for this call as model creation would run it, into a block that is freed again.
 * DCS_EUNSUPPORTED for the column-filter graphs (kw == 1: never folded), DCS_EINVAL when n_out is short.  Synchronises the
 * stream. */
DCS_API int dcs_debug_conv_fold_weights(const dcs_model* m, float* out_h, int64_t n_out, int64_t* rows, int64_t* cols);

/* Test aids for the decoder kernels of the DSD graphs (csrc/dsd.hip, dsd_bf16x3.hip, dsd_lat.hip; tests/test_gpu_dsd_kernels.py);
 * no reference counterpart.  dcs_debug_dsd_stage runs ONE decoder stage of a DSD or stereo (ILD) model on the caller's buffers
 * with the model's own packed weights (Bw2, Bw2s, Bw2q, Lw2p, Bfin, Bpk, bout, the cross-fade ramp):
 *   DCS_DSD_STAGE_DECONV2  D [n_items][h2][52] floats -> G [n_items][7][tc][8] floats and / or Gs [n_items][7][tc][3][8] bf16
 *   DCS_DSD_STAGE_FINAL    G or Gs of n tiles per clip, three (four: stereo model) branches per tile, and the mixture rows ->
 *                          out: source s of clip c at out + c * out_clip_stride + s * out_src_stride, rows of out_ld floats
 * family = DCS_DSD_FAMILY_THROUGHPUT: dcs_launch_dsd_deconv2 / dcs_launch_dsd_final as the separation paths call them, so the
 * choice of kernel is the production one (G is required as they always carve it; Gs is optional; no_bq != 0 withholds the bf16
 * planes of the conv2 weights, as a model without them would).  DCS_DSD_FAMILY_ONE_BATCH: dcs_launch_lat_deconv2 (G, Gs or both) /
 * dcs_launch_lat_final (Gs).  The final stage fills the launcher's arguments as dcs_separate* / dcs_model_forward_masked /
 * dcs_separate_stereo do: fold != 0: rows frames are folded from n tiles that start tc - ov frames apart, mixture x scale;
 * fold == 0: rows = n * tc rows of the tiles themselves (ov ignored).  n_clips > 1: clip c reads its G at tile c * g_clip_tiles and
 * its mixture at mix + c * mix_clip_stride; clip_tab_h (nullable, HOST, six int64 per clip {samples, frames, tiles, row offset,
 * tile offset, rows}) is checked against the buffers and uploaded for the call (row offsets all < 0: the pitches above apply;
 * all >= 0: the compact layout).  DCS_EINVAL, and nothing launched, for a null, misaligned (16 bytes) or short buffer -- every
 * byte count must cover what the separation paths would carve for the same dimensions -- and for dimensions out of range;
 * what the launchers refuse comes back as they return it, nothing launched either.  One stream synchronisation per call. */
#define DCS_DSD_STAGE_DECONV2 0
#define DCS_DSD_STAGE_FINAL 1
#define DCS_DSD_FAMILY_THROUGHPUT 0
#define DCS_DSD_FAMILY_ONE_BATCH 1
typedef struct dcs_debug_dsd_args {
    int32_t family, no_bq;
    const float* D; int64_t D_bytes;
    float* G; int64_t G_bytes;
    void* Gs; int64_t Gs_bytes;
    const float* mix; int64_t mix_bytes; int64_t mix_ld;
    float* out; int64_t out_bytes; int64_t out_ld, out_src_stride;
    int64_t n_items;                      /* deconv2: (tile, branch) items */
    int64_t n, rows;                      /* final: tiles and output rows per clip (the maxima with a clip table) */
    int32_t ov, fold, mask_mode; float scale;
    int32_t n_clips; int64_t g_clip_tiles, mix_clip_stride, out_clip_stride;
    const int64_t* clip_tab_h;
} dcs_debug_dsd_args;
DCS_API int dcs_debug_dsd_stage(dcs_model* m, int stage, dcs_debug_dsd_args* args);
/* Which kernel each role of the model's context launched last (any entry point; 0 = none since the last dcs_debug_dsd_stage
 * began, which clears them): codes[DCS_DSD_ROLES], and the launchers' choices params[DCS_DSD_PARAMS] = {X, Xt (workgroup
 * columns per full / for the partial channel group of a streaming deconv2), waves per workgroup, deconv2 workgroups, cbw,
 * n_colg, final workgroups per clip, mmax}.  Host-side bookkeeping, one store per launch.  Every pointer but m is nullable. */
#define DCS_DSD_ROLE_DECONV2 0
#define DCS_DSD_ROLE_GSPLIT 1
#define DCS_DSD_ROLE_FINAL 2
#define DCS_DSD_ROLES 3
#define DCS_DSD_PARAMS 8
#define DCS_DSD_K_DECONV2 1               /* deconv2_kernel<13> */
#define DCS_DSD_K_DECONV2_STREAM 2        /* deconv2_stream_kernel<false> */
#define DCS_DSD_K_DECONV2_STREAM_SPLIT 3  /* deconv2_stream_kernel<true> */
#define DCS_DSD_K_DECONV2_BF16_4 4        /* deconv2_stream_bf16_kernel<4> */
#define DCS_DSD_K_DECONV2_BF16_16 5       /* deconv2_stream_bf16_kernel<16> */
#define DCS_DSD_K_GSPLIT 6                /* g_split_kernel */
#define DCS_DSD_K_LAT_DECONV2 7           /* lat_deconv2_kernel */
#define DCS_DSD_K_FINAL 8                 /* final_kernel<FOLD, MODE, CBW, 3>: 8 + (FOLD * 3 + MODE) * 2 + CBW - 1 = 8 .. 19 */
#define DCS_DSD_K_FINAL4 20               /* final_kernel<FOLD, MODE, 1, 4>: 20 + FOLD * 2 + MODE - 2 = 20 .. 23 */
#define DCS_DSD_K_FINAL_BF16X3 24         /* final_bf16x3_kernel<MODE>: 24 + MODE */
#define DCS_DSD_K_LAT_FINAL 26            /* lat_final_kernel<MODE>: 26 + MODE */
DCS_API int dcs_debug_dsd_last_kernel(const dcs_model* m, int* codes, int64_t* params);

/* Test aids for the kernels of the deep score-informed graph build_ca_1x1 (csrc/deep1x1_igemm.h, deep1x1.hip, train_deep1x1.hip;
 * tests/test_gpu_d1_kernels.py); no reference counterpart.  dcs_debug_d1_conv runs ONE d1::launch<MODE> -- one instance of
 * d1_igemm_kernel<MODE, NT> -- on the caller's buffers for a geometry the caller gives; no model is needed.  The launch
 * arguments are filled by the helpers the separator and the trainer fill theirs with (d1::forward_args / transposed_args), and
 * the launch comes from the translation unit that launches that mode in production: DCS_D1_FWD, _1X1, _TR, _LAST from
 * deep1x1.hip (with trainer_unit != 0, FWD and TR from the trainer's copy), DCS_D1_FWDC, _Q, _B11 from train_deep1x1.hip.
 *   forward type (FWD, 1X1, FWDC)  in [images][Hi][Wi][Ci] channels-last; a valid kh x kw convolution with column stride
 *                                  `stride`; Ho = Hi - kh + 1 and Wo = (Wi - kw) / stride + 1 are returned
 *   transposed type (TR, LAST, Q, B11)  the transpose of the valid kh x kw convolution (kw == 5: stride 2; kw == 1: stride 1,
 *                                  par 0) that took [Ho][Wo] to [Hi][Wi]; in and code [images][Hi][Wi][Ci]; one launch writes the
 *                                  output columns of parity par.  Ho, Wo are the caller's: Hi == Ho - kh + 1, Wi == (Wo - kw) / stride + 1
 * B is [Npad][Kpad] floats, Npad = N rounded up to 16 NT (NT = 1, 2, 4 for N <= 16, <= 32, above), Kpad = K rounded up to 16,
 * K = kh ntap Ci, zero past K and past row N.  Outputs as D1Args documents them: FWD / FWDC / B11 [M][Co]; TR
 * [images][Ho][Wo][Co]; 1X1 [N / 200 branches][M][200]; Q [images][N][Ho][Wo]; LAST [ch_off + N][n_total][Ho][Wo], this call's
 * images from tile k_first.  code: r'(pre) bytes 0 / 1 / 2 of `in` (transposed type) or of `out` (FWDC, [M][Co]).
 * DCS_EINVAL, and nothing launched, for a null pointer the mode uses, a pointer not aligned to 16 bytes, a byte count below what
 * the geometry reads or writes, M == 0 (a parity without a column), a channel pitch (Ci, Co) that is not a multiple of 4,
 * Co below N or above Npad, a contiguous K run (kw Ci floats of a forward type, Ci floats of a transposed type) below the 16
 * that D1Args requires, and geometry out of range.  One stream synchronisation per call. */
#define DCS_D1_FWD 0
#define DCS_D1_1X1 1
#define DCS_D1_TR 2
#define DCS_D1_LAST 3
#define DCS_D1_FWDC 4
#define DCS_D1_Q 5
#define DCS_D1_B11 6
typedef struct dcs_debug_d1_args {
    int32_t images, Hi, Wi, Ci;
    int32_t Ho, Wo;                       /* transposed type: given; forward type: returned */
    int32_t kh, kw, stride, par;
    int32_t N, Co;
    int64_t n_total, k_first; int32_t ch_off;     /* LAST */
    int32_t trainer_unit;
    const float* in; int64_t in_bytes;
    const uint8_t* code; int64_t code_bytes;
    const float* B; int64_t B_bytes;
    const float* b0; int64_t b0_bytes;    /* FWD, 1X1, LAST, Q: N floats */
    const float* b1; int64_t b1_bytes;    /* FWD, 1X1: N floats */
    float* out; int64_t out_bytes;
    uint8_t* code_out; int64_t code_out_bytes;    /* FWD: [M][Co] bytes */
    int32_t nt, grid_x, grid_y, K, Kpad, Wq;      /* returned: the instance, its grid and the launch's K, Kpad, Wq */
    int64_t M;                            /* returned */
} dcs_debug_d1_args;
DCS_API int dcs_debug_d1_conv(dcs_ctx* ctx, int mode, dcs_debug_d1_args* args);
/* The small kernels around it and the two weight packers, with the same checks (every pointer a device pointer):
 *   DCS_D1_AUX_TO_CL       d1_to_cl_kernel: in [n][4][plane] -> out [n][plane][4]
 *   DCS_D1_AUX_MASK        d1_mask_kernel: in p [4][n][plane], in2 x [n][C][plane] -> out [4][n_total][plane] from tile k_first;
 *                          mode DCS_EPS_A / DCS_EPS_B, the mixture the sum of the first mix_n channels of x
 *   DCS_D1_AUX_CODE_APPLY  code_apply_kernel on nsum workgroups of `per` rows: out [rows][Cp] *= 0.5 in2 (code bytes [rows][Cp])
 *                          in place; out2 (nullable) [nsum][C] the column sums of out as it was
 *   DCS_D1_AUX_CODES_OUT   codes_out_kernel: in code bytes [n][hw][Cp] -> out [n][C][hw] floats
 *   DCS_D1_AUX_PACK_HOST   the separator's host packer: in W [Cout][Cin][kh][kw] (Lasagne) -> out B, out2 Bt[0], out3 Bt[1],
 *                          written whole (pads zero); kw 5 or 1 (kw == 1: out3 unused)
 *   DCS_D1_AUX_PACK_DEVICE the trainer's pack_kernel: in W [kh][kw][Cin][Cout] (internal) -> the live elements of out, out2, out3;
 *                          everything else is left as it was */
#define DCS_D1_AUX_TO_CL 0
#define DCS_D1_AUX_MASK 1
#define DCS_D1_AUX_CODE_APPLY 2
#define DCS_D1_AUX_CODES_OUT 3
#define DCS_D1_AUX_PACK_HOST 4
#define DCS_D1_AUX_PACK_DEVICE 5
typedef struct dcs_debug_d1_aux_args {
    int64_t n, plane, n_total, k_first, rows, per, hw;
    int32_t C, Cp, mode, mix_n, nsum;
    int32_t Cin, Cout, kh, kw;
    const void* in; int64_t in_bytes;
    const void* in2; int64_t in2_bytes;
    void* out; int64_t out_bytes;
    void* out2; int64_t out2_bytes;
    void* out3; int64_t out3_bytes;
} dcs_debug_d1_aux_args;
DCS_API int dcs_debug_d1_aux(dcs_ctx* ctx, int which, dcs_debug_d1_aux_args* args);

/* Test aids for the training GEMM and its helper kernels (csrc/train_core.h, train_core.hip, train_debug.hip;
 * tests/test_gpu_train_kernels.py); no reference counterpart.  dcs_debug_train_gemm runs ONE dcs_trainer::launch(g, tile, ak, bk)
 * -- one instance of train::gemm_kernel -- on the caller's buffers; no model and no trainer is needed.  The arguments carry what
 * train::Gemm carries; the Gemm is built with gemm0, ax3 and mat, the helpers the graph files use.  An operand is a pointer, its
 * byte count, an element offset and two axes, each (d0, d1, s0, s1, s2): index i is at (i % d0) s0 + (i / d0 % d1) s1 +
 * (i / (d0 d1)) s2, d0 d1 clipped at 2^30.  tile: DCS_TRAIN_T128X32, _T64X64, _T32X32; ak / bk: the operand is loaded K-fastest.
 * Before the launch the aid computes, for every operand the launch uses and every batch, the smallest and largest element the
 * descriptor addresses over its index range (A: rows below min(M, ones_row); C and X are not used with `partial`, X only with
 * DCS_TRAIN_EPI_SAVEPRE / _DRELU; bias, bias2 and scale may be null).  DCS_EINVAL, and nothing launched, for a null or
 * 16-byte-misaligned pointer the launch uses, a byte count below that extent, an element below the pointer, a negative stride
 * (the aid's extent is for non-negative strides; production's one negative stride, the flipped conv2 weights of train_ca.hip's
 * F5 / B5, is outside it), d0 or d1 outside 1 .. 2^30, M, N or K outside 1 .. 2^30 - 1, nbatch outside 1 .. 4, splits < 1,
 * splits > 1 without `partial` or with a kchunk that is not a positive multiple of 32, nbatch splits above 65535,
 * DCS_TRAIN_EPI_SAVEPRE together with _DRELU, epi bits outside the three, and an unknown tile.  grid_x, grid_y, grid_z return the
 * grid dcs_trainer::launch used.  One stream synchronisation per call. */
#define DCS_TRAIN_T128X32 0
#define DCS_TRAIN_T64X64 1
#define DCS_TRAIN_T32X32 2
#define DCS_TRAIN_EPI_RELU 1
#define DCS_TRAIN_EPI_SAVEPRE 2
#define DCS_TRAIN_EPI_DRELU 4
typedef struct dcs_debug_train_mat {
    float* p; int64_t bytes;
    int64_t off;
    int64_t r[5], c[5];                   /* rows and columns (A: M, K; B: K, N; C and X: M, N): d0, d1, s0, s1, s2 */
} dcs_debug_train_mat;
typedef struct dcs_debug_train_gemm_args {
    int32_t M, N, K;
    int32_t tile, ak, bk;
    dcs_debug_train_mat A, B, C, X;
    int32_t ones_row, ones_klim;          /* rows >= ones_row of A read 1 for k < ones_klim, else 0 */
    int32_t nbatch, bias_cs;
    int64_t boff[4][5];                   /* per batch: offsets of A, B, C, X, bias */
    const float* bias; int64_t bias_bytes;
    const float* bias2; int64_t bias2_bytes;
    const float* scale; int64_t scale_bytes;
    int32_t epi, splits, kchunk;
    int32_t grid_x, grid_y, grid_z;       /* returned */
    float* partial; int64_t partial_bytes;        /* [nbatch splits][M][N] */
} dcs_debug_train_gemm_args;
DCS_API int dcs_debug_train_gemm(dcs_ctx* ctx, dcs_debug_train_gemm_args* args);
/* One launch of a helper, with the same refusals for null, misaligned or short buffers (every pointer a device pointer):
 *   DCS_TRAIN_AUX_FINISH           dcs_trainer::finish (finish_kernel) on a trainer of B rows: in part [splits][B][N], in2 bias [N]
 *                                  (nullable), out C [B][N], out2 X [B][N] (with DCS_TRAIN_EPI_SAVEPRE written, with _DRELU read)
 *   DCS_TRAIN_AUX_REDUCE           dcs_trainer::reduce (reduce_kernel), two jobs: in / in2 part [splits[j]][count[j]], in3 the
 *                                  scale, out / out2 dst: count[j] floats, and N[j] more where dup[j] (the last N[j] once more);
 *                                  count[1] == 0: one job
 *   DCS_TRAIN_AUX_DECONV1_IKALA    train::deconv1_kernel<30, 30, 3, 2>, the launch of train_ikala.hip
 *   DCS_TRAIN_AUX_DECONV1_BACH10   train::deconv1_kernel<30, 30, 4, 4>, the launch of train_bach10.hip
 *   DCS_TRAIN_AUX_DECONV1_BACH10SI train::deconv1_channels_kernel<30, 30, 4, 4>, the launch of train_bach10si.hip
 *                                  in g [B][tc][w1][30] per source, source k at + k gslot (BACH10SI: one slot); in2 W1i [30][30]
 *                                  (BACH10SI [4][30][30]); in3 bo per source / channel; out q [B][sources][tc][F];
 *                                  F >= 30 and w1 == (F - 30) / S1 + 1, the graph's */
#define DCS_TRAIN_AUX_FINISH 0
#define DCS_TRAIN_AUX_REDUCE 1
#define DCS_TRAIN_AUX_DECONV1_IKALA 2
#define DCS_TRAIN_AUX_DECONV1_BACH10 3
#define DCS_TRAIN_AUX_DECONV1_BACH10SI 4
typedef struct dcs_debug_train_aux_args {
    int32_t B, N, splits, epi;            /* FINISH */
    int64_t count[2];                     /* REDUCE */
    int32_t rsplits[2], rN[2], dup[2];
    int32_t tc, F, w1, pad_;              /* DECONV1 (with B) */
    int64_t gslot;
    const float* in; int64_t in_bytes;
    const float* in2; int64_t in2_bytes;
    const float* in3; int64_t in3_bytes;
    float* out; int64_t out_bytes;
    float* out2; int64_t out2_bytes;
} dcs_debug_train_aux_args;
DCS_API int dcs_debug_train_aux(dcs_ctx* ctx, int which, dcs_debug_train_aux_args* args);

/* Test aids for the one-batch kernels of csrc/dsd_lat.hip (csrc/lat_debug.hip; tests/test_gpu_lat_kernels.py); no reference
 * counterpart.  Each runs ONE launch through the launcher net.hip calls (dcs_launch_lat_gemm, dcs_launch_lat_stft,
 * dcs_launch_lat_istft) on the caller's device buffers, after the host has computed the highest element the launch can ask of
 * every buffer; one stream synchronisation per call.
 *
 * dcs_debug_lat_gemm: lat_gemm_kernel<J, NA>, J = ceil(slice_len / 16), NA = a_parts.  The fields are DcsLatGemm's (csrc/dsd_lat.h):
 *   nz <= 1:  C[r][c] = act(a_scale * Aeff[arow(r)][0 .. K) . B[:, c] + bias[c]),  r < M, c < n_store, rows of ldc floats
 *   nz > 1 :  part z at C + z * c_part_stride holds the sum over the slices z * waves .. z * waves + waves - 1 alone,
 *             waves = ceil(n_slices / nz); the bias in part 0 only; no rectifier
 *   Aeff = the sum of the a_parts arrays a_part_stride apart, rectified if relu_in; arow(r) = a_gdiv > 0 ? (r / a_gdiv) * a_gmul +
 *   r % a_gdiv : r, rows a_row_stride apart (they may overlap); Bp in the fragment order of dcs_lat_pack_b_host.
 * Extents: A: max_r arow(r) * a_row_stride + K + (a_parts - 1) * a_part_stride floats (and the first four floats of every part,
 * which lanes without an operand read); Bp: n_slices * n_cb * J * 256; bias: n_cb * 16 (read past n_store); C: (nz - 1) *
 * c_part_stride + (M - 1) * ldc + n_store.  DCS_EINVAL, and nothing launched, for a count below its extent, a pointer that is
 * null or not 16-byte aligned, a negative stride or count (M, n_store, K, n_slices, n_cb below 1; M above 2^20), n_store above
 * n_cb * 16 or above ldc, c_part_stride below one part while nz > 1, and everything the launcher refuses: waves outside 4 .. 16,
 * slice_len, K, a_row_stride or a_part_stride not a multiple of 4, slice_len above 80 (J > 5), a_parts other than 1 or 4.
 * J, NA, grid_* and block_x return the launch. */
typedef struct dcs_debug_lat_gemm_args {
    const float* A; int64_t n_A; int64_t a_row_stride;
    const float* Bp; int64_t n_Bp;
    const float* bias; int64_t n_bias;
    float* C; int64_t n_C; int64_t ldc;
    float a_scale;
    int32_t M, n_store, K, slice_len, n_slices, n_cb, relu;
    int32_t nz, a_parts, relu_in, a_gdiv;
    int64_t c_part_stride, a_part_stride, a_gmul;
    int32_t J, NA, grid_x, grid_y, grid_z, block_x;   /* returned */
} dcs_debug_lat_gemm_args;
DCS_API int dcs_debug_lat_gemm(dcs_ctx* ctx, dcs_debug_lat_gemm_args* args);
/* lat_stft_kernel<9 | 10> (frameSize 1024 / 2048, frameSize / hop 2 or 4, else DCS_EINVAL): T = dcs_frame_count(n_samples, hop)
 * frames of audio_d[0 .. n_samples) into rows_out >= T rows of ld >= frame / 2 + 1 values: magnitudes, angles (phase_d nullable)
 * and unit phasors ((re, im) pairs); rows past T and the columns past frame / 2 are written as magnitude 0, angle 0, phasor
 * (1, 0).  n_audio: floats behind audio_d (n_samples <= n_audio); n_rows_elems: elements (pairs for unit_d) behind every output,
 * at least rows_out * ld.  audio_d, mag_d and phase_d may be aligned to 4 bytes only (an audio_d off 8 bytes takes the kernel's
 * scalar loads), unit_d to 8. */
DCS_API int dcs_debug_lat_stft_forward_f32(dcs_stft* plan, const float* audio_d, int64_t n_audio, int64_t n_samples, float* mag_d,
                                           float* phase_d, float* unit_d, int64_t n_rows_elems, int64_t ld, int64_t rows_out);
/* lat_ifft_kernel<9 | 10, 4> and lat_ola_kernel<2 | 4>: source s reads n_frames rows of ld magnitudes at mag_d + s * src_stride
 * and the shared phasor rows at unit_d, X = (mag / pre_div) * sqrt(frame) * unit with the imaginary parts of bins 0 and frame / 2
 * ignored; the windowed frames go to frames_d [n_src][n_frames][frame] (the caller's, so that they can be looked at), the
 * overlap-add / sum of window^2 to audio_d [n_src][n_out]; samples no frame covers are 0.  n_mag, n_audio: floats; n_unit:
 * pairs.  DCS_EINVAL for frames_bytes below n_src * n_frames * frame * 4, ld < frame / 2 + 1, src_stride < n_frames * ld with
 * more than one source, n_mag < (n_src - 1) * src_stride + (n_frames - 1) * ld + frame / 2 + 1, n_unit < (n_frames - 1) * ld +
 * frame / 2 + 1, n_audio < n_src * n_out, a count below 1, pre_div 0 or not finite, a null or misaligned pointer (mag_d, audio_d
 * 4 bytes, unit_d, frames_d 8). */
DCS_API int dcs_debug_lat_stft_inverse_f32(dcs_stft* plan, const float* mag_d, int64_t n_mag, int64_t src_stride, const float* unit_d,
                                           int64_t n_unit, int64_t ld, int64_t n_frames, int n_src, float pre_div, float* audio_d,
                                           int64_t n_audio, int64_t n_out, float* frames_d, int64_t frames_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DCS_H */
