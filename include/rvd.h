/* rvd.h -- C ABI of the MI355X-native diarization hot path (same shared library as rvb.h: librvb.so).
 *
 * What it replaces.  /root/reference/diarization/infer_pyannote3.0.py:33-42 builds
 * `pyannote.audio.Pipeline.from_pretrained("Revai/reverb-diarization-v1")`, moves it to the GPU and
 * calls `pipeline(audio)`.  Inside that call the two neural networks are the hot path:
 *
 *   segmentation   PyanNet (SincNet + 4 x BiLSTM(128) + 2 x Linear(128) + 7-class powerset head) on every
 *                  10 s window, hop 1 s        (pyannote.audio Inference.slide -> model.forward)
 *   embedding      WeSpeaker ResNet34 + masked statistics pooling on every (window, local speaker) pair
 *
 * The glue between them (powerset decoding, speaker counting, clustering, reconstruction, RTTM) is host
 * code in reverb_amd/diarization.py.  A maintainer binds this header with ctypes exactly as
 * reverb_amd/_lib.py does (INTEGRATION.md shows the pyannote-side stub).
 *
 * Conventions: every function returns 0 on success or a negative RVB_E_* code (rvb.h); the message is in
 * rvd_last_error().  Host pointers are plain C arrays.  All tensors are loaded as fp32 in the layout and
 * under the names of the pyannote checkpoints' state dicts, prefixed "segmentation." / "embedding.".
 * There is no CPU fallback: rvd_create fails when no HIP device is present.
 */
#ifndef RVD_H
#define RVD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rvd_engine rvd_engine;

typedef struct rvd_model_cfg {
  int32_t struct_size;      /* sizeof(rvd_model_cfg) in the caller's binding; rvd_create refuses any other value (rvb.h) */
  int32_t dtype;            /* RVB_F32 (0) exact-parity mode, RVB_BF16 (1) bf16 MFMA inputs, fp32 accumulate, RVB_FP8 (2) = the
                               bf16 engine with the 3x3 convolutions of the embedding trunk's stages 3-4 on e4m3 operands
                               (BASELINE configs[4]; scales calibrated by the first rvd_embed call, see rvd_get_emb_fp8) */
  int32_t sample_rate;      /* 16000 */
  int32_t window_samples;   /* 160000 (10 s) */
  int32_t step_samples;     /* 16000  (segmentation_step 0.1 x window) */
  int32_t sinc_filters;     /* 80 (40 cos + 40 sin), kernel 251, stride 10 */
  int32_t sinc_channels;    /* 60: Conv1d(80,60,5), Conv1d(60,60,5) */
  int32_t lstm_hidden;      /* 128 (bidirectional) */
  int32_t lstm_layers;      /* 4 */
  int32_t linear_dim;       /* 128 */
  int32_t linear_layers;    /* 2 */
  int32_t num_classes;      /* 7 powerset classes (3 speakers, <= 2 simultaneously) */
  int32_t emb_channels;     /* 32: ResNet34 m_channels; 0 = no embedding model loaded */
  int32_t emb_dim;          /* 256 */
} rvd_model_cfg;

const char* rvd_last_error(void);
int rvd_model_cfg_size(void);   /* sizeof(rvd_model_cfg) of this build */
/* distinct windows one pass of the embedding trunk takes (768 unless RVD_EMB_BATCH says otherwise; halved by rvd_embed when the
 * activations of that many windows -- 35 MB each in bf16 -- cannot be allocated): a host that prepares pooling masks underneath
 * the first pass (reverb_amd/diarization.py) needs the masks of exactly this many windows up front */
int rvd_emb_windows_per_pass(rvd_engine* e);

int rvd_create(const rvd_model_cfg* cfg, int device, rvd_engine** out);
void rvd_destroy(rvd_engine* e);
/* stage one fp32 tensor of a checkpoint, e.g. "segmentation.sincnet.conv1d.1.weight" */
int rvd_load_tensor(rvd_engine* e, const char* name, const float* host, const int64_t* shape, int ndim);
/* pack weights for the device (sinc filters from low_hz_/band_hz_, conv weights as GEMM operands,
 * BatchNorm folded into the ResNet convolutions) and free the staged copies */
int rvd_finalize(rvd_engine* e);

/* windows pyannote's Inference.slide makes of n samples: the full ones plus one zero-padded tail */
int64_t rvd_num_windows(const rvd_engine* e, int64_t n_samples);
/* frames the segmentation model emits per window (589 for 10 s) */
int rvd_frames_per_window(const rvd_engine* e);

/* 16-bit mono PCM at cfg.sample_rate -> HBM; evaluates the sinc filter bank once for all windows */
int rvd_upload_pcm(rvd_engine* e, const int16_t* pcm, int64_t n_samples);
/* n_rec recordings in one upload and one front-end pass, packed so that the kernels see one long recording.  Recording r has
 * W_r = rvd_num_windows(n_samples[r]) windows and takes (W_r + window_samples / step_samples - 1) * step_samples samples (its own
 * zero-padded length) from sample first_window[r] * step_samples on: its window w is GLOBAL window first_window[r] + w, which is
 * the index rvd_segment_windows, rvd_embed and rvd_get_emb_fbank take, and every such window sees exactly the samples and zeros it
 * sees after rvd_upload_pcm of that recording alone (results are bit-identical).  The window_samples / step_samples - 1 global
 * indices between two recordings straddle a boundary: never list them.  *total_windows = one past the last valid global index.  A
 * recording of 0 samples has no windows and takes no space (its first_window is that of the next recording).  n_rec < 1, a null
 * pointer for a non-empty recording or a negative length: RVB_E_ARG.  rvd_rerun_resident afterwards reruns the packed front end;
 * rvd_upload_pcm returns the engine to a single recording. */
int rvd_upload_pcm_many(rvd_engine* e, const int16_t* const* pcm, const int64_t* n_samples, int n_rec,
                        int64_t* first_window /* [n_rec] */, int64_t* total_windows);
/* the recording of the last rvd_upload_pcm is still resident in HBM: run its front end again (everything rvd_upload_pcm does
 * behind the copy -- waveform, sinc filter bank, embedding fbank).  For callers that keep a recording on the device and for
 * bench_diar.py, whose timed step starts from HBM-resident samples as the ASR bench's does (the reference has no counterpart:
 * pyannote re-reads the file, diarization/infer_pyannote3.0.py:37). */
int rvd_rerun_resident(rvd_engine* e);
/* pyannote's `Audio` resamples every file to the model's rate (torchaudio.functional.resample with its defaults = the kernel of
 * the ASR front end, rvb_upload_pcm_rate): int16 mono PCM at `sample_rate` -> int16 at cfg.sample_rate, on the device.
 * out == NULL: only *n_out is written; otherwise *n_out holds the capacity of `out` on entry, the length on return. */
int rvd_resample_pcm(rvd_engine* e, const int16_t* pcm, int64_t n_samples, int sample_rate, int16_t* out, int64_t* n_out);

/* segmentation model on windows [first, first+n): logp_out host fp32 [n][frames][num_classes] (NULL: keep the
 * result on the device only) */
int rvd_segment(rvd_engine* e, int64_t first_window, int n_windows, float* logp_out);
/* rvd_segment over a window LIST: row i of the result (and of what rvd_get_classes / rvd_get_tap return afterwards) is window
 * windows[i] (after rvd_upload_pcm_many: a global index).  An index outside the uploaded audio is refused before anything runs.
 * A window's result does not depend on the call or the row it is computed in. */
int rvd_segment_windows(rvd_engine* e, const int64_t* windows, int n, float* logp_out);
/* argmax powerset class of every frame of the last rvd_segment (what Powerset.to_multilabel(soft=False) needs):
 * out host uint8 [n][frames] */
int rvd_get_classes(rvd_engine* e, uint8_t* out);
/* debug taps of the last rvd_segment over n windows, as stored (fp32 copies; pad columns included).  Reads only: nothing
 * rvd_segment computes depends on them.  Rows per window: p1 = ((window_samples - 251) / 10 + 1) / 3, p2 = (p1 - 4) / 3,
 * frames = (p2 - 4) / 3; CP = 64, the padded width of the sinc_channels-wide tensors.
 *   "sincnet"   [n][frames][sinc_channels]   the SincNet output without its pad columns
 *   "lstm"      [n][frames][2*hidden]        the last LSTM layer's output
 *   "a1"        [n][p1][sinc_filters]        block 1 output
 *   "c2"        [n][p1][CP]                  conv 2 output; the last 4 rows of a window are never read and hold whatever the
 *   "c3"        [n][p2][CP]                  convolution made of the next window's frames or of the buffer's slack: ignore them
 *   "a2"        [n][p2][CP]   "a3" [n][frames][CP]      block 2 / 3 outputs
 *   "lstm_prev" [n][frames][2*hidden]        the last LSTM layer's input (needs lstm_layers >= 2)
 *   "linear0", "linear1" [n][frames][linear_dim]   outputs of linear layers 0 and 1, where no later layer reuses their buffer
 *                                            (at most 2 / 3 linear layers)
 *   "stats"     [n][2]                       every window's waveform mean and 1 / sqrt(var + eps), fp32 as the first block reads them
 *   "fsum"      [sinc_filters]               the sums of the sinc filters' taps, fp32 as the first block reads them
 *   "craw"      [(n_pad - 251) / 10 + 1][sinc_filters]   the sinc convolution of the whole upload,
 *                                            n_pad = (windows - 1) * step_samples + window_samples
 * n is the window count of that rvd_segment call: the caller's buffer must hold that many windows. */
int rvd_get_tap(rvd_engine* e, const char* name, float* out);

/* embedding model: for each of n items, window index win[i] and a frame mask[i][frames] (weights in [0,1],
 * resampled to the ResNet's time axis as pyannote does); emb_out host fp32 [n][emb_dim] */
int rvd_embed(rvd_engine* e, const int64_t* win, const float* mask, int n, float* emb_out);
/* debug: the 80-bin log-mel features of one window as fed to the ResNet, [frames][80]; returns frames in *n */
int rvd_get_emb_fbank(rvd_engine* e, int64_t window, float* out, int32_t* n_frames);
/* Parity taps of the embedding pass (read-only; for the tests' stage-by-stage check of the ResNet34 trunk, whose three rotating
 * buffers per stage keep nothing of a block).  rvd_set_emb_tap(e, 1) makes every later TRUNK PASS of rvd_embed copy its stored
 * tensors, device to device on the engine's stream, into buffers the engine owns; the taps hold the LAST pass (rvd_embed runs one
 * pass per rvd_emb_windows_per_pass() distinct windows).  Off (0, the default) releases them, and rvd_embed enqueues exactly what it
 * enqueues without this entry point.  rvd_get_emb_tap copies one tensor out: bf16 widened to fp32 bit for bit, fp32 as it is;
 * `capacity` = floats `out` can take.  With B windows and n items in the pass, stage s = 1..4 of F_s x T_s pixels (80 x 998, 40 x 499,
 * 20 x 250, 10 x 125 for 10 s windows) and C_s = 32, 64, 128, 256 channels, block b = 0.. of that stage:
 *   "feats"    [B][T_1][80]    fp32   the fbank frames of the pass's windows, before mean subtraction
 *   "mean"     [B][80]         fp32   their per-window means, as the stem reads them
 *   "stem"     [B][F_1 + 2][T_1 + 2][C_1]     the stem's output; like every tensor below WITH its zero border of one pixel
 *   "s<s>b<b>.x"    the block's input as it stood when the block read it ([B][F + 2][T + 2][C] of the stage it comes from)
 *   "s<s>b<b>.tmp"  its first convolution's output -- not stored by a block that runs as one kernel (conv_block.hip)
 *   "s<s>b<b>.sc"   its projection shortcut's output -- only where the shortcut is stored (not when it rides in the second convolution's K loop)
 *   "s<s>b<b>.out"  its output
 *   "trunk"    [B][F_4 + 2][T_4 + 2][C_4]     what the pooling reads
 *   "stats"    [n][2 C_4 F_4]                 the pooled statistics, as seg_1 reads them
 *   "windows"  [B]  "item_b" [n]              the pass's window list and every item's row in it (integers as floats)
 *   "forms"    [3 + 3 x 16]    B, the first item of the pass, n, then per block (stage-major): the kernel of its first and of its second
 *              convolution (1 direct, 2 implicit GEMM, 3 row64, 4 stream, 5 implicit GEMM on the wide tile, 6 the one-kernel block, 7 the
 *              stride-2 opener) and where its shortcut went (0 identity, 1 a launch of its own, 2 the stride-2 opener, 3 the K loop)
 * Refused by name, with nothing written: rvd_set_emb_tap(e, 1) on an fp8 engine or with RVD_EMB_FP8=1 (RVB_E_UNSUPPORTED); a pass of
 * rvd_embed over more than 4 windows while the taps are on (RVB_E_UNSUPPORTED); rvd_get_emb_tap before any such pass, or for a name
 * the last pass did not keep (RVB_E_STATE); a buffer that is too small (RVB_E_ARG). */
int rvd_set_emb_tap(rvd_engine* e, int enabled);
int rvd_get_emb_tap(rvd_engine* e, const char* name, float* out, int64_t capacity);

/* clustering step of the pipeline: the dendrogram scipy.cluster.hierarchy.linkage(X, method="centroid",
 * metric="euclidean") returns for X host fp64 [n][d] -- Z host fp64 [n-1][4] (id_a, id_b, distance, size),
 * rows in merge order, cluster n+k created by row k.  fp64 throughout. */
int rvd_centroid_linkage(rvd_engine* e, const double* X, int n, int d, double* Z);
/* rvd_centroid_linkage for many point sets at once: X host fp64 [sum n][d], the problems back to back; n [n_problems]; Z host fp64
 * [sum max(n - 1, 0)][4], back to back, cluster ids per problem (0 .. 2 n[p] - 2).  Problems of fewer than 3 000 points share one
 * device allocation, one distance-matrix launch, one nearest-neighbour launch and one merge-loop launch in which every problem
 * has a workgroup of its own; each dendrogram is what rvd_centroid_linkage gives for that problem with one workgroup
 * (rvd_set_linkage_workgroups(e, 1)), bit for bit.  Larger problems go through rvd_centroid_linkage one by one.  n[p] < 2 gives no
 * rows.  A problem in which no pair can be merged (non-finite points) fails the call with RVB_E_ARG; the message names its index. */
int rvd_centroid_linkage_many(rvd_engine* e, const double* X, const int32_t* n, int n_problems, int d, double* Z);
/* How many workgroups the merge loop of rvd_centroid_linkage may take (it is persistent: its workgroups keep their CUs for the
 * whole clustering): 0 = default (16 workgroups of one XCD from 3 000 points on), 1 = one workgroup, 2 / 4 / 8 / 16.  The
 * dendrogram does not depend on it.  A pipeline that clusters UNDERNEATH another engine's kernels (transcribe_diarize: the ASR
 * encoder) asks for 4: measured on one hour, joint step 472 ms with 4, 477 with 1, 486 with 8, 493-499 with 16. */
int rvd_set_linkage_workgroups(rvd_engine* e, int workgroups);
/* Round 4 CANDIDATE (compiled, not yet run on a GPU): with RVD_EMB_FP8=1 in the environment at rvd_finalize, stages 3-4 of the ResNet34
 * trunk (the MFMA-bound half of the embedding network) run on e4m3 operands (csrc/conv_gemm.hip conv_igemm8_kernel): weights scaled
 * per output channel at load, activations per tensor at scales calibrated by the FIRST trunk pass of the engine (which runs in bf16).
 * *state: 0 = off or not calibrated, 1 = calibrating, 2 = active; scales (nullable; *n in: capacity, out: 32) = the activation
 * scales, index ((stage - 2) * 8 + block) * 2 + {0: first convolution's output, 1: block output}; *clipped (nullable) = values that
 * did not fit e4m3 at those scales so far. */
int rvd_get_emb_fp8(rvd_engine* e, int32_t* state, float* scales, int32_t* n, uint32_t* clipped);
/* Install the 32 activation scales (layout as rvd_get_emb_fp8) and make the fp8 path active at once: every later trunk pass runs on
 * e4m3 operands at these scales, no bf16 calibration pass.  How the ranks of a sharded run agree on ONE quantisation of the
 * recording (reverb_amd/dist.py diarize_sharded: each rank calibrates on its windows, the element-wise maximum is installed
 * everywhere and the windows are embedded again), as rvb_set_fp8_scales does on the ASR side.  The clip counter restarts. */
int rvd_set_emb_fp8_scales(rvd_engine* e, const float* scales, int32_t n);

int rvd_set_profiling(rvd_engine* e, int enabled);
int rvd_reset_timings(rvd_engine* e);
int rvd_get_timing(rvd_engine* e, const char* name, double* ms, double* flops, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
