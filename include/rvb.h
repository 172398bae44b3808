/* librvb -- C ABI of the MI355X-native Reverb-ASR hot path (gfx950 HIP kernels behind it).
 *
 * The reference (revdotcom/reverb) is pure Python and exposes no FFI; its boundary for the
 * `recognize_wav` hot path is the Python API in asr/wenet/cli/reverb.py and the inner seam
 * `ASRModel.decode` (asr/wenet/transformer/asr_model.py:331-432).  Each entry point below names
 * the reference interface it replaces.  The Python host in reverb_amd/ binds these with ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions: plain C, opaque handle, every function returns 0 (RVB_OK) or a negative RVB_E*
 * code; rvb_last_error() returns the calling thread's last error string.  Host buffers are
 * caller-owned; device memory is library-owned.  One engine per device; an engine is not
 * thread-safe, distinct engines are.  All device work runs on the engine's own HIP stream and
 * every function returns after its results are complete on the host.
 */
#ifndef RVB_H_
#define RVB_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVB_OK 0
#define RVB_E_ARG -1
#define RVB_E_HIP -2
#define RVB_E_STATE -3
#define RVB_E_NOMEM -4
#define RVB_E_UNSUPPORTED -5
#define RVB_E_TIMEOUT -7        /* a collective did not complete within rvb_comm_set_timeout (-6: corrupt audio data) */

#define RVB_F32 0  /* parity mode: v_mfma_f32_16x16x4_f32, exact f32 fma chains */
#define RVB_BF16 1 /* throughput mode: v_mfma_f32_16x16x32_bf16, fp32 accumulate/residual */
#define RVB_FP8 2  /* BASELINE configs[4]: the bf16 engine with the encoder's feed-forward GEMMs (rvb_set_fp8_policy: also qkv / pointwise-conv) on
                      v_mfma_scale_f32_32x32x64_f8f6f4 (OCP e4m3 operands: weights scaled per output channel, activations per
                      tensor, scales calibrated by the FIRST rvb_encode call, which itself runs in bf16) */

typedef struct rvb_engine rvb_engine;

/* Model dimensions: the values the reference reads from config.yaml
 * (asr/wenet/utils/init_model.py:102-183; cli/reverb.py:62-98). */
typedef struct rvb_model_cfg {
  int32_t struct_size;   /* sizeof(rvb_model_cfg) as the CALLER's binding lays it out: rvb_create refuses any other value
                            (RVB_E_ARG, "ABI mismatch"), so a binding written against an older header -- a field short, as
                            INTEGRATION.md's stub was after round 3 added cnn_causal -- fails by name instead of making the
                            library read past the caller's struct */
  int32_t dtype;         /* RVB_F32 | RVB_BF16 | RVB_FP8 */
  int32_t input_dim;     /* input_dim (80 mel bins) */
  int32_t vocab;         /* output_dim */
  int32_t d_model;       /* encoder_conf.output_size */
  int32_t heads;         /* encoder_conf.attention_heads */
  int32_t ffn_dim;       /* encoder_conf.linear_units */
  int32_t num_blocks;    /* encoder_conf.num_blocks (first and last are language-specific if num_langs>0) */
  int32_t cnn_kernel;    /* encoder_conf.cnn_module_kernel (odd unless cnn_causal) */
  int32_t cnn_norm;      /* 0 layer_norm, 1 batch_norm (encoder_conf.cnn_module_norm) */
  int32_t num_langs;     /* dataset_conf.cat_emb_conf.emb_len when pass_cat_emb, else 0 */
  int32_t dec_heads;     /* decoder_conf.attention_heads */
  int32_t dec_ffn_dim;   /* decoder_conf.linear_units */
  int32_t dec_blocks;    /* decoder_conf.num_blocks   (left decoder) */
  int32_t dec_r_blocks;  /* decoder_conf.r_num_blocks (right decoder, 0 = none) */
  int32_t blank_id;      /* ctc_conf.ctc_blank_id */
  int32_t sos_id;        /* vocab-1 (asr_model.py:79-82) */
  int32_t eos_id;
  int32_t max_chunks;    /* chunks per device batch (workspace sizing) */
  int32_t chunk_frames;  /* max input frames per chunk (2051, cli/reverb.py:188) */
  int32_t cnn_causal;    /* encoder_conf.causal: the convolution module pads cnn_kernel-1 frames on the left only
                            (convolution.py:55-57,113-121) and carries a cnn cache across streamed chunks */
} rvb_model_cfg;

const char* rvb_last_error(void);
const char* rvb_version(void);
/* sizeof(rvb_model_cfg) of THIS build: what a binding's struct_size has to equal (a binding can assert it at load) */
int rvb_model_cfg_size(void);

/* ReverbASR.__init__ / init_model / load_checkpoint (cli/reverb.py:46-98,
 * utils/init_model.py:99-277, utils/checkpoint.py:29-80): create an engine, stream the
 * state-dict tensors in by their reference names (fp32, host memory), then finalize. */
int rvb_create(const rvb_model_cfg* cfg, int device, rvb_engine** out);
void rvb_destroy(rvb_engine* e);
int rvb_load_tensor(rvb_engine* e, const char* name, const float* host, const int64_t* shape, int ndim);
/* Fold the language-specific linear layers with `cat_embs` = [verbatimicity, 1-verbatimicity]
 * (cli/reverb.py:215-217; encoder_layer.py:378-390, decoder_layer.py:319-330), pack weights to
 * the compute dtype, precompute the per-layer positional keys.  May be called again with other
 * cat_embs.  Fails listing the first missing tensor. */
int rvb_finalize(rvb_engine* e, const float* cat_embs, int n_cat);

/* Same for PCM at another sample rate: resampled on the device to 16 kHz the way the reference does
 * (asr/wenet/cli/reverb.py:128-134: `torchaudio.transforms.Resample(sr, 16000)` on the float waveform =
 * sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99); the fbank then reads the un-rounded float result. */
int rvb_upload_pcm_rate(rvb_engine* e, const int16_t* pcm, int64_t n_samples, int sample_rate);
/* the waveform the fbank will read (after resampling, int16 scale); out may be NULL to query the length */
int rvb_get_waveform(rvb_engine* e, float* out, int64_t* n_samples);

/* ReverbASR.compute_feats (cli/reverb.py:119-146): Kaldi fbank of 16 kHz mono int16 PCM.
 * rvb_upload_pcm copies the samples to HBM; rvb_fbank computes [n_frames,80] log-mel on the
 * device (kept resident, zero-padded to whole chunks) and optionally copies it to feats_out.  With feats_out == NULL the
 * call only enqueues the kernel (rvb_encode is ordered behind it on the engine's stream); with a host buffer it returns
 * when the copy has landed. */
int64_t rvb_num_frames(int64_t n_samples);
/* ReverbASR.compute_feats with front-end settings OTHER than the model's 80 bins / 25 ms / 10 ms (cli/reverb.py:119-146 passes
 * num_mel_bins, frame_length, frame_shift straight to kaldi.fbank; its own default is 23 bins): stand-alone, not bound to an engine.
 * wave: mono waveform at 16 kHz on the int16 scale (what `.to(torch.float)` of the loaded file holds), host memory; feats_out
 * [n_frames][num_mel_bins] (NULL: only *n_frames is set).  Supported: frame_length 16.1 .. 32 ms (Kaldi pads the window to the
 * next power of two: the 512-point FFT of the hot path), any frame_shift, 1 .. 128 bins, dither 0; RVB_E_UNSUPPORTED otherwise. */
int rvb_compute_feats(int device, const float* wave, int64_t n_samples, int num_mel_bins, double frame_length_ms,
                      double frame_shift_ms, float* feats_out, int64_t* n_frames);
int rvb_upload_pcm(rvb_engine* e, const int16_t* pcm, int64_t n_samples);
/* Page-locked host memory for the audio reader (what `torchaudio.load` fills in the reference, cli/reverb.py:128):
 * PCM decoded straight into such a buffer reaches HBM at the PCIe rate (115 MB per hour of audio in ~2 ms);
 * pageable memory works with rvb_upload_pcm too, several times slower.  Free with rvb_host_free. */
/* Double-buffered upload for back-to-back recordings (a long-form service decodes file i while file i+1 arrives): the copy
 * is enqueued on a copy stream of the engine's and the call returns at once; from page-locked memory it runs on a DMA engine
 * underneath the decoding in progress.  The samples become the engine's audio at the NEXT rvb_fbank, which orders itself
 * behind the copy on the device; `pcm` must stay valid and unchanged until that rvb_fbank has been called and one more
 * stream synchronisation (any blocking call) has passed.  One upload may be pending at a time (RVB_E_STATE otherwise).
 * 16 kHz int16 only.  Replaces: the `torchaudio.load` + `.to(device)` of the NEXT file in cli/reverb.py:128-146, which the
 * reference runs serially. */
int rvb_upload_pcm_async(rvb_engine* e, const int16_t* pcm, int64_t n_samples);
int rvb_host_alloc(void** out, int64_t bytes);
int rvb_host_free(void* p);
int rvb_fbank(rvb_engine* e, float* feats_out /* nullable [n_frames*80] */, int64_t* n_frames);

/* The audio reader itself -- `torchaudio.load(audio_file, normalize=False)` followed by `.to(torch.float)`
 * (asr/wenet/cli/reverb.py:128-130) -- for the lossless containers, decoded on the host from a file image in memory
 * (csrc/audio.cpp).  normalize=False keeps the decoder's native sample format, so the VALUES depend on the container:
 *   RIFF/WAVE  PCM 16 (int16), PCM 8 (uint8, 0..255 as stored), PCM 24 / 32 (int32; 24-bit left-justified = value << 8),
 *              IEEE float 32 / 64 (as stored), A-law / mu-law (expanded to int16); WAVE_FORMAT_EXTENSIBLE and RF64 of the same
 *   AIFF / AIFF-C  NONE / twos / sowt PCM 8 (signed in the file, handed on as uint8 = value + 128) / 16 / 24 / 32, fl32 / fl64, alaw / ulaw
 *   FLAC       (RFC 9639) <= 16 bits per sample: int16, left-justified; wider: int32, left-justified; frame CRC-8 / CRC-16
 *              and the STREAMINFO MD5 of the decoded PCM are verified (md5_checked = 1 when the file carries a signature)
 *   MPEG audio Layer III (MP3; MPEG-1, MPEG-2 and 2.5 sampling rates, mono / stereo / joint stereo, CRC checked when present): float32,
 *              full scale 1.0; a leading Xing / Info / VBRI frame is skipped and the encoder delay / padding of a LAME-style tag are trimmed
 *              the way FFmpeg (torchaudio's loader) trims them; free format and Layers I / II are refused by name
 * Ogg is refused by name (RVB_E_UNSUPPORTED); corrupt data is -6.
 * rvb_audio_probe fills `info` only.  The decode calls write channel `channel` (or, with channel = -1, all channels
 * planar [channels][frames]) into `out` of `capacity` samples and return the frames per channel (< 0: error code).
 * flags: RVB_AUDIO_NO_MD5 skips the FLAC signature check (the loader of the reference does not check it either); bits 8..15 =
 * host threads for FLAC (0 = one per 512 KiB of stream, at most 16: frames decode independently, a 1 h file in ~0.1 s).
 * rvb_audio_decode_i16 serves the files whose native format is int16 (sample_format == RVB_SAMPLE_I16): the PCM can go
 * straight into a page-locked buffer for rvb_upload_pcm_rate; everything else goes through rvb_audio_decode_f32 and
 * rvb_upload_wave_f32. */
enum { RVB_AUDIO_WAVE = 1, RVB_AUDIO_FLAC = 2, RVB_AUDIO_AIFF = 3, RVB_AUDIO_MP3 = 4 /* MPEG-1 / 2 / 2.5 audio Layer III: float32 */ };
enum { RVB_AUDIO_NO_MD5 = 1 };
enum { RVB_SAMPLE_U8 = 1, RVB_SAMPLE_I16 = 2, RVB_SAMPLE_I32 = 3, RVB_SAMPLE_F32 = 4, RVB_SAMPLE_F64 = 5 };
typedef struct rvb_audio_info {
  int32_t container;        /* RVB_AUDIO_* */
  int32_t sample_format;    /* RVB_SAMPLE_*: the dtype of the tensor torchaudio would return */
  int32_t channels;
  int32_t sample_rate;
  int32_t bits_per_sample;  /* as the file declares it */
  int32_t md5_checked;
  int64_t frames;           /* samples per channel */
  int32_t decode_threads;   /* host threads the decode used (FLAC: runs of frames) */
  int32_t reserved;
} rvb_audio_info;
int rvb_audio_probe(const void* data, int64_t nbytes, rvb_audio_info* info);
int64_t rvb_audio_decode_f32(const void* data, int64_t nbytes, int channel, float* out, int64_t capacity, int flags, rvb_audio_info* info);
int64_t rvb_audio_decode_i16(const void* data, int64_t nbytes, int channel, int16_t* out, int64_t capacity, int flags, rvb_audio_info* info);
/* rvb_upload_pcm_rate for a float waveform (`waveform.to(torch.float)` of a non-int16 source, cli/reverb.py:130-134):
 * resampled on the device when sample_rate != 16000; the fbank reads the float values as they are. */
int rvb_upload_wave_f32(rvb_engine* e, const float* wave, int64_t n_samples, int sample_rate);

/* Several recordings resident together: what the reference's bin/recognize.py does with a data set -- batches through the same
 * model.decode -- for the users who transcribe thousands of short recordings.  N recordings cost one upload call, ONE fbank launch
 * and ceil(chunks / max_chunks) rvb_encode calls, and each recording keeps the frames (snip_edges per recording: no frame reads a
 * neighbour's samples), the chunks and the zero padding it has when uploaded alone, so its results are those of the single calls.
 *
 * rvb_batch_plan: host only, no engine.  The layout the other calls use, from the 16 kHz lengths n_samples [n_rec]: n_frames [n_rec],
 * first_chunk [n_rec + 1] = the chunk row each recording starts at (first_chunk[n_rec] = all chunks; a recording under 400 samples
 * has no frame and no chunk: equal neighbours) and, when asked for, lens [first_chunk[n_rec]] = the valid frames of every chunk
 * (chunk_size, the recording's last chunk its remainder: feats_batcher, cli/reverb.py:148-180).  Call it once with lens = NULL to
 * size lens.  chunk_size >= 7 (RVB_E_ARG); 1 <= n_rec <= 65 536 (more: RVB_E_UNSUPPORTED naming the cap).
 *
 * rvb_upload_batch: data[r] holds n_samples[r] mono samples, int16 (sample_format[r] == RVB_SAMPLE_I16) or float at int16 scale
 * (RVB_SAMPLE_F32), at sample_rate[r] (1000 .. 384000; other than 16000: resampled on the device as rvb_upload_pcm_rate /
 * rvb_upload_wave_f32 do, one launch per such recording).  16 kHz int16 recordings are packed into one int16 device buffer, float
 * recordings and the resampler's outputs into one float buffer.  Returns when the copies have landed.  Every argument is checked
 * before any device work (RVB_E_ARG naming the recording; the cap on n_rec as above).  A batch upload replaces a single upload
 * and the other way round; while an rvb_upload_pcm_async upload is pending the call is refused (RVB_E_STATE).
 * rvb_batch_n_samples: the 16 kHz lengths [n_rec] after resampling, which rvb_batch_plan needs.
 *
 * rvb_fbank_batch: one launch of the segmented fbank kernel over the live frames of all recordings; recording r's frame j goes to
 * row first_chunk[r] * chunk_size + j of the resident features, every other row of its chunks is zero, and
 * rvb_encode(e, NULL, first_chunk, lens, B, chunk_size, ...) then reads any chunk range, also one that crosses recordings.
 * 7 <= chunk_size <= cfg.chunk_frames.  n_frames [n_rec] and first_chunk [n_rec + 1] are filled as by rvb_batch_plan; feats_out
 * (nullable) receives all first_chunk[n_rec] * chunk_size rows of 80.  RVB_E_STATE, naming the right call: rvb_fbank_batch
 * without rvb_upload_batch, and rvb_fbank or rvb_get_waveform on a batch. */
int rvb_batch_plan(const int64_t* n_samples, int n_rec, int chunk_size, int64_t* n_frames /* [n_rec] */,
                   int64_t* first_chunk /* [n_rec+1] */, int32_t* lens /* nullable [first_chunk[n_rec]] */);
int rvb_upload_batch(rvb_engine* e, const void* const* data, const int32_t* sample_format, const int64_t* n_samples,
                     const int32_t* sample_rate, int n_rec);
int rvb_batch_n_samples(rvb_engine* e, int64_t* out /* [n_rec] */);
int rvb_fbank_batch(rvb_engine* e, int chunk_size, float* feats_out /* nullable [total_chunks*chunk_size*80] */, int64_t* n_frames,
                    int64_t* first_chunk);

/* Chunks cut at pauses, chosen on the device (csrc/pause_chunks.hip).  The calls above cut a recording every chunk_size frames, as
 * the reference's feats_batcher does, which usually lands inside a word.  rvb_pause_chunks moves each cut to the quietest place of
 * the `search` frames before that boundary.  THE DEFINITION, per recording, over its own n fbank frames f = 0 .. n-1 (nothing reads
 * a neighbour recording's rows):
 *   loudness  e[f] = the fp32 sum of the 80 log-mel values of frame f.  s[c], for a cut position c in 0 .. n (the cut lies between
 *             frames c-1 and c), = the fp32 sum of e[clamp(c+j, 0, n-1)] for j = -h .. h-1; h = the smoothing half-width, 1 <= h <= 64
 *             (10 = 200 ms is the default of the Python layers).  e is formed as ONE sum of 80 terms and s as ONE sum of 2h values
 *             of e, in any order within each sum; no running or prefix sums across frames.
 *   pieces    start_0 = 0.  While n - start_k > chunk_size: lo = start_k + chunk_size - search, hi = min(start_k + chunk_size, n - 7),
 *             start_{k+1} = the LAST c in [lo, hi] that attains the minimum of s; a NaN s is never chosen, and if every candidate is
 *             NaN the cut is hi.  The final piece runs to n.  lens[k] = start_{k+1} - start_k.
 *   search    the frames before the fixed boundary in which a cut may fall, 7 <= search <= chunk_size - 7 (the Python layers default
 *             to chunk_size / 4).  Then every piece but a recording's only one has at least 7 frames, none exceeds chunk_size, and
 *             lo <= hi always.  A recording with n <= chunk_size is one piece, identical to the fixed chunk; n = 0 gives no piece.
 *   ties      the last minimum cuts as late as possible (fewer chunks); exact ties are common: digital silence gives every bin the
 *             floor value -15.942385.
 * Valid after rvb_fbank (one recording) or rvb_fbank_batch (n_rec recordings; the chunk_size here need not be that call's).  Three
 * kernels (frame loudness, cut search: one workgroup per recording, gather) and one copy of the small start table to the host.
 * Piece k's rows go to chunk row k * chunk_size of a SECOND feature buffer, the rest of the slot zero; pieces of all recordings are
 * numbered consecutively in recording order.  Outputs: first_chunk [n_rec + 1] = each recording's first piece (first_chunk[n_rec] =
 * *n_chunks = all pieces), starts [*n_chunks] = each piece's first frame within its recording, lens [*n_chunks]; feats_out
 * (nullable) receives the *n_chunks * chunk_size packed rows of 80.  From then on rvb_encode(e, NULL, first_chunk, lens, B,
 * chunk_size, ...) reads the packed buffer.  The frame-ordered features are kept: a second call with other parameters works from
 * them.  The next upload or fbank call restores the fixed layout.
 * Checked before any device work, by name: RVB_E_ARG for h or search out of range and for chunk_size outside [7, cfg.chunk_frames];
 * RVB_E_STATE when no features are resident; RVB_E_NOMEM naming the bytes.  capacity = the entries of starts and lens: if the cuts
 * give more pieces (at most ceil(n / (chunk_size - search)) per recording) the call returns RVB_E_ARG naming the count, *n_chunks
 * holds it, nothing else is written and the layout stays as it was.  Timed under "pause_chunks" in rvb_get_timing, one launch group
 * per call (the bracket holds the three kernels and the table copy between them). */
int rvb_pause_chunks(rvb_engine* e, int chunk_size, int search, int h, int64_t* first_chunk /* [n_rec+1] */, int32_t* starts,
                     int32_t* lens, int64_t capacity, int64_t* n_chunks, float* feats_out /* nullable */);
/* Back to the fixed layout without a new fbank call: rvb_encode(e, NULL, ...) reads the frame-ordered features again (host only). */
int rvb_fixed_chunks(rvb_engine* e);

/* Chunk-masked encoder attention for the following rvb_encode calls: query frame i attends the encoder frames
 * [max((i/chunk - left)*chunk, 0), (i/chunk + 1)*chunk) -- what `decoding_chunk_size` / `num_decoding_left_chunks`
 * select in BaseEncoder.forward via add_optional_chunk_mask (encoder.py:140-145, utils/mask.py:86-197) for models
 * trained with use_dynamic_chunk / static_chunk_size.  chunk_size <= 0: full context (default); left < 0: all. */
int rvb_set_decoding_chunk(rvb_engine* e, int chunk_size, int num_left_chunks);

/* RVB_FP8 engines: which GEMM groups of which conformer blocks run on the fp8 MFMA path -- `groups` is a bit mask (1 macaron
 * feed-forward, 2 qkv projection, 4 pointwise conv 1, 8 pointwise conv 2, 16 feed-forward) applied to the blocks
 * first_block .. last_block (last_block < 0: the last one), plus 32 = the subsampling's second convolution (not per block;
 * rvb_get_fp8_subsample); everything else stays bf16.  groups < 0 restores the default: the
 * feed-forward modules of every block (17), the policy whose token error rate against the reference stays at the level of the
 * reference's own bf16 autocast (tests/test_fp8_gpu.py).  Takes effect with the next rvb_encode; call after rvb_finalize. */
int rvb_set_fp8_policy(rvb_engine* e, int groups, int first_block, int last_block);

/* ASRModel._forward_encoder + ctc_logprobs + per-frame top-`beam` (asr_model.py:288-329,378-389,
 * search.py:155): encode a batch of B chunks of T0 frames.  feats: host fp32 [B,T0,80], or NULL
 * to read chunk rows [first_chunk, first_chunk+B) of the device-resident rvb_fbank output.
 * lens: valid input frames per chunk (feats_batcher, cli/reverb.py:148-180). */
int rvb_encode(rvb_engine* e, const float* feats, int64_t first_chunk, const int32_t* lens, int B, int T0,
               int beam, float blank_penalty);
/* Streaming encoder: BaseEncoder.forward_chunk / forward_chunk_by_chunk (asr/wenet/transformer/encoder.py:231-402) for
 * one stream.  rvb_stream_begin empties the attention cache; rvb_stream_chunk encodes one chunk of `n_frames` input frames
 * ((chunk-1)*4 + 7 for a full chunk, encoder.py:378-381) against the cached keys / values of earlier chunks, positional keys
 * at absolute frame positions, and keeps the last `required_cache_size` frames (< 0: all, 0: none) as forward_chunk does;
 * `out` (nullable) receives the chunk's encoder output [n_out, d] fp32.  The caches live in the engine (the reference
 * returns att_cache / cnn_cache tensors): per block the key|value rows of the cached frames and, for a causal convolution
 * module (cnn_causal), the pointwise-conv1 outputs of the last cnn_kernel-1 frames -- the reference's cnn_cache holds the
 * module inputs of those frames and pushes them through pointwise_conv1 again with every chunk (convolution.py:113-125).
 * rvb_stream_finish runs the CTC head + top-k over all frames produced and makes them the current batch (one "chunk"), so
 * that rvb_ctc_greedy / rvb_ctc_prefix_beam / rvb_attention_rescore / rvb_get_encoder_out work on the streamed output --
 * ASRModel.decode(simulate_streaming=True) (asr_model.py:301-306). */
int rvb_stream_begin(rvb_engine* e);
int rvb_stream_chunk(rvb_engine* e, const float* feats, int n_frames, int required_cache_size, float* out, int32_t* n_out);
int rvb_stream_state(rvb_engine* e, int32_t* offset, int32_t* cache_frames);
int rvb_stream_finish(rvb_engine* e, int beam, float blank_penalty);
int rvb_encoder_frames(rvb_engine* e, int32_t* T_out);                 /* encoder frames per chunk (512) */
int rvb_get_encoder_lens(rvb_engine* e, int32_t* lens /* [B] */);      /* encoder_mask.sum (asr_model.py:387) */
int rvb_get_encoder_out(rvb_engine* e, float* out /* [B,T,d] */);      /* parity tap */
int rvb_get_ctc_logprobs(rvb_engine* e, int chunk, float* out /* [T,V] */); /* parity tap */
int rvb_get_ctc_topk(rvb_engine* e, float* vals, int32_t* idx /* [B,T,beam] each */);
/* Parity taps of ONE position of the offline encoder (tests only; read-only: what rvb_encode computes does not change).  The encoder
 * reuses its workspaces in every block, so nothing of a block survives the call; with a position selected -- block = 0 .. blocks - 1
 * for a conformer block, block = blocks for the front end before block 0, -1 for off (the default) -- the following rvb_encode calls
 * copy every stored tensor of that position, device to device on the engine's stream, into buffers the engine owns.  M = B * T rows:
 *   block:     x_in x_ffm x_att x_conv x_ff x_out [M][d] fp32 (the residual stream on entry and after each module, the block's
 *              output); xn_ffm xn_mha xn_conv xn_cnn xn_ff next [M][d], h_ffm h_ff [M][ff], qkv [M][3d], ao dconv [M][d],
 *              glu [M][d] (GLU in the GEMM's epilogue) or [M][2d], y [M][d] (language-specific blocks only): the compute dtype;
 *              pos_keys [T][d] (compute dtype) and pos_bias [heads][T] fp32 (bf16 engines) as loaded
 *   front end: X1 [B][T1][F1][d], X2 [B][T][F2][d], xn0 [M][d] (compute dtype), x0 [M][d] fp32
 *   forms:     forms[0] = n, then n small integers -- block: K' = k + p written by the qkv GEMM (1 / 0), GLU in the epilogue (1 / 0),
 *              then for every GEMM in launch order (ffm1 ffm2 qkv att_out pw1 pw2 [lsl] ff1 ff2; front end: conv2 embed) 2 if
 *              gemm() handed it to gemm2.hip, else 1
 * rvb_get_encoder_tap copies one out: bf16 widened to fp32 bit for bit, fp32 as it is; `capacity` = floats `out` can take.
 * Refused by name, with nothing written: rvb_set_encoder_tap on an fp8 engine (RVB_E_UNSUPPORTED) or with a stream open
 * (RVB_E_STATE); rvb_encode of a batch that is encoded in two slices (B >= 16) and rvb_stream_chunk while a position is selected
 * (RVB_E_UNSUPPORTED); a name the last rvb_encode did not keep (RVB_E_STATE).  Off, rvb_encode enqueues exactly what it does
 * without this switch; switching off or to another position frees the kept copies. */
int rvb_set_encoder_tap(rvb_engine* e, int block);
int rvb_get_encoder_tap(rvb_engine* e, const char* name, float* out, int64_t capacity);
/* The same for ONE position of one rescoring decoder (tests only; read-only): side 0 = left, 1 = right decoder; position 0 ..
 * layers - 1 = that decoder layer, `layers` = the head (final norm, output layer, log-softmax gather), -1 = off (the default).  With a
 * position selected, every following pass of that decoder over a prefix trie -- rvb_attention_rescore and rvb_attention_score;
 * rvb_attention_decode and rvb_joint_decode run other code and ignore the switch -- copies every stored tensor of the position,
 * device to device on the engine's stream.  R = trie rows, M = B * T encoder frames, P = (hypothesis, position) pairs:
 *   layer:  x_in x_self x_src x_ff [R][d] fp32 (the residual stream on entry and after self attention, cross attention and the feed
 *           forward); xn1 xn2 xn3 [R][d], qkv [R][3d], ao_self ao_src q [R][d], y [R][d] (language-specific layers only), h [R][ff],
 *           kvmem [M][2d] (the layer's memory keys | values, made by rvb_prepare_rescoring or by the call): the compute dtype;
 *           layer 0 also x_emb [R][d] fp32, the embedding's output
 *   head:   x_in [R][d] fp32, xn_after [R][d] (compute dtype), logits [R][(V + 3) & ~3] fp32 (kept only while R <= 8192, one logit
 *           slab; refused by name beyond), logp [P] fp32 in slot order (tgt_ptr)
 *   trie:   the batch as the host built it, int32 carried in floats: 13, the lengths of the 13 arrays, then the arrays tok pos path
 *           hq_start hq_len hq_pos0 hkv_start hkv_len crow_start crow_len tgt_ptr tgt work (trie_dims: those first 14 values alone)
 *   forms:  forms[0] = n, then n integers in launch order -- per GEMM of the position 2 (gemm2.hip) or 1 (gemm.hip), per attention the
 *           eight of its kernel instantiation (element size, padded dk, positional keys, waves, fold, key pad, occupancy, fragments):
 *           layer = qkv, self attention, self_out, src_q, cross attention, src_out, [language mix,] ff1, ff2; head = the output layer
 *           once per logit slab.  (The memory K/V GEMM runs before the layers, or in rvb_prepare_rescoring: not listed.)
 * Refused by name with nothing written and the kept copies untouched: a position on an fp8 engine (RVB_E_UNSUPPORTED), a side or
 * position out of range (RVB_E_ARG), a name the last pass did not keep (RVB_E_STATE), a buffer too small (RVB_E_ARG).  Off, the decoder
 * enqueues exactly what it does without this switch; switching off, to another position or side frees the kept copies. */
int rvb_set_decoder_tap(rvb_engine* e, int side, int position);
int rvb_get_decoder_tap(rvb_engine* e, const char* name, float* out, int64_t capacity);

/* ctc_greedy_search (search.py:106-121): tokens [B,T] (first ntok[b] valid) and the frame of each
 * token's first emission. */
int rvb_ctc_greedy(rvb_engine* e, int32_t* tokens, int32_t* ntok, int32_t* frames);

/* Forced alignment of a KNOWN transcript: force_align (asr/wenet/utils/ctc_utils.py:105-161) as bin/alignment.py:233-242 calls it
 * on `model.ctc.log_softmax(encoder_out)` -- CTC Viterbi of the given token ids over the log-probs (no blank penalty) of the chunks
 * of the last rvb_encode / rvb_stream_finish, on the device (csrc/ctc_viterbi.hip; fp32 adds and comparisons only, so the labels equal
 * the reference's for the same log-prob bits, ties included).
 * n_seq sequences; sequence i aligns tokens [sum tok_lens[..i), +tok_lens[i]) against the VALID encoder frames
 * (rvb_get_encoder_lens) of the chunks first_chunk[i] .. first_chunk[i] + n_chunks[i] - 1, concatenated: n_chunks = 1 is the
 * reference's utterance-by-utterance use, one sequence over every chunk aligns the transcript of a whole recording.  Frames are
 * numbered within the sequence.  Outputs (each nullable): labels [sum of the sequences' frames], concatenated: the token id or
 * the blank id per frame; per token (concatenated like `tokens`): begin / end = first / last frame of the token's run, peak = the
 * frame of that run with the largest log-prob of the token (first on ties), confidence = exp of that log-prob; score [n_seq] = the
 * fp32 path score.  Refused by name (RVB_E_ARG) where the reference's output is undefined: an empty transcript, ids outside
 * [0, vocab) or equal to the blank, a transcript the frames cannot emit (fewer frames than tokens + adjacent repeats, or no path
 * with a finite score).  Caps per sequence (RVB_E_UNSUPPORTED, before any device work; rvb_ctc_align_limits): */
#define RVB_CTC_ALIGN_MAX_TOKENS 16383      /* 32 767 lattice states (the reference's int16 back-pointers break there, silently) */
#define RVB_CTC_ALIGN_MAX_FRAMES 1048576    /* 11.6 h at 40 ms; back-pointers take 2 bits per frame and state of device memory
                                               (RVB_E_NOMEM if they do not fit) */
int rvb_ctc_align(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* first_chunk,
                  const int32_t* n_chunks, int32_t* labels, int32_t* begin, int32_t* end, int32_t* peak, float* confidence,
                  float* score);
int rvb_ctc_align_limits(int32_t* max_tokens, int32_t* max_frames);

/* rvb_ctc_align for a transcript with GAPS: RVB_CTC_WILDCARD in `tokens` is a position that stands for "some audio that was not
 * transcribed" (the <star> token of torchaudio's aligner).  It is an ordinary CTC label with an id of its own: it stays, is entered
 * from the blank before it or from the token two states below, two adjacent wildcards need a blank between them like any repeated
 * token, it takes AT LEAST ONE frame, and it counts as a token towards the caps and towards frames >= tokens + adjacent repeats.
 * Its emission at frame t is w[t] + wildcard_bias in fp32, w[t] = the largest log-prob of the frame over all vocab columns, the
 * blank included: a wildcard frame costs what the model's own greedy path costs there, so a wildcard absorbs speech and silence
 * alike and never beats a token the model agrees with (it ties; ties go to the first maximum in the order stay, one below, two
 * below).  wildcard_bias <= 0 (RVB_E_ARG if positive or not finite) is a penalty per wildcard frame in nats: the wildcard is used
 * only where the transcript misfits by more than that.  A leading / trailing wildcard gives a free start / end.
 * Arguments, outputs, caps and refusals are those of rvb_ctc_align; `labels` holds RVB_CTC_WILDCARD on a wildcard's frames, its
 * peak is the frame of its run with the largest w (first on ties) and its confidence exp of that w (without the bias).  With no
 * wildcard among the tokens every output is bit-identical to rvb_ctc_align's, which itself still refuses the id as outside
 * [0, vocab).  rvb_ctc_score has no wildcards: a full-sum score of a transcript with gaps is not defined here. */
#define RVB_CTC_WILDCARD (-2)
int rvb_ctc_align_wild(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* first_chunk,
                       const int32_t* n_chunks, float wildcard_bias, int32_t* labels, int32_t* begin, int32_t* end, int32_t* peak,
                       float* confidence, float* score);

/* LONG-FORM alignment: ONE transcript of any number of tokens over a recording that is encoded in several batches (a WINDOWED
 * Viterbi, csrc/ctc_viterbi_window.hip).  At every frame only W consecutive states of the lattice are alive, the window; it follows
 * the best partial path, moves only between kernel launches and never back.  With W >= 2 n_tokens + 1 it never moves and every
 * output is rvb_ctc_align_wild's, bit for bit; otherwise the result is the best path among those that stay inside the windows, and
 * min_margin tells how close that path came to a window edge (in states; an edge that is the lattice's own does not count; W when
 * none counts).  A margin of 0 says the true path may have been cut off: align again with a wider window.
 *   begin   tokens may hold RVB_CTC_WILDCARD (wildcard_bias finite and <= 0, as for rvb_ctc_align_wild).  total_frames = the valid
 *           encoder frames of ALL batches to come (<= RVB_CTC_ALIGN_MAX_FRAMES, RVB_E_UNSUPPORTED above).  window_states: 0 (the
 *           default, 32 768 = 16 384 tokens) or a multiple of 256 in [256, 32768]; reduced to the lattice rounded up to 32 states.
 *           Refusals in rvb_ctc_align's words, all before any device work; no token cap beyond n_tokens + repeats <= total_frames.
 *           Back-pointers take total_frames x W / 4 bytes (RVB_E_NOMEM naming them).  begin while a lattice is open replaces it.
 *   feed    after rvb_encode: every valid frame of every chunk of the encoded batch, in order, continues the lattice (the log-probs
 *           are recomputed in the slabs rvb_encode used, as rvb_ctc_align does).  RVB_E_STATE before begin, before rvb_encode, or
 *           when the batch holds more frames than the lattice has left.  rvb_ctc_align*, _score and _find stay usable in between.
 *   finish  RVB_E_STATE unless exactly total_frames were fed.  labels [total_frames], begin / end [n_tokens] as rvb_ctc_align
 *           defines them over the whole lattice, score, min_margin (each nullable).  RVB_E_ARG "infeasible: no path inside the
 *           window ..." when the score is -inf; outputs are then untouched.
 *   emissions  lp[t][labels[t]] of the valid frames of the encoded batch (n_frames of them; a RVB_CTC_WILDCARD frame: the row
 *           maximum), for peaks and confidences: encode the batches a second time and pass each its part of finish's labels.
 *   end     releases the buffers. */
int rvb_ctc_align_long_limits(int32_t* max_frames, int32_t* max_window_states, int32_t* default_window_states);
int rvb_ctc_align_long_begin(rvb_engine* e, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states,
                             float wildcard_bias);
int rvb_ctc_align_long_feed(rvb_engine* e);
int rvb_ctc_align_long_finish(rvb_engine* e, int32_t* labels, int32_t* begin, int32_t* end, float* score, int32_t* min_margin);
int rvb_ctc_align_long_emissions(rvb_engine* e, const int32_t* labels, int n_frames, float* emit_out);
int rvb_ctc_align_long_end(rvb_engine* e);

/* LONG-FORM full-sum score: rvb_ctc_score (loglik, and with posteriors the per-token occupancy, mean frame, peak posterior and its
 * frame) of ONE transcript of any number of tokens over a recording that is encoded in several batches (a WINDOWED forward-backward,
 * csrc/ctc_fb_window.hip).  The window, its policy and its limits (rvb_ctc_align_long_limits) are the long alignment's, except that the
 * window follows the first maximum of the normalised forward row over the states that can still reach the end.
 * Band semantics.  lo_of[t], the window of the launch that computes frame t, is a multiple of 32 and never decreases.  Cell (t, s) is
 * alive iff lo_of[t] <= s < min(lo_of[t] + W, S).  A transition (t-1, s') -> (t, s) counts iff both cells are alive and
 * s' >= lo_of[t].  loglik is the full sum over the paths made of counted transitions (<= the full sum of the whole lattice), and the
 * posteriors are those of that sum: over the alive states of a frame they add up to 1.
 * Bit-identity.  With W >= 2 n_tokens + 1 rounded up to 32 the window never moves: loglik and all four per-token outputs are then
 * rvb_ctc_score's bit for bit, however the batches cut the recording.
 *   begin      tokens as rvb_ctc_score's (RVB_CTC_WILDCARD is an id outside the vocabulary); total_frames, window_states and the
 *              refusals as rvb_ctc_align_long_begin's, all before any device work.  posteriors != 0 keeps the forward rows,
 *              total_frames x W x 4 bytes (RVB_E_NOMEM naming them).  begin while a lattice is open replaces it.
 *   feed       after rvb_encode, batches in ASCENDING order: every valid frame of every chunk continues the forward sweep.
 *              RVB_E_STATE before begin, before rvb_encode, or when the batch holds more frames than the lattice has left.
 *   loglik     RVB_E_STATE unless exactly total_frames were fed.  RVB_E_ARG "infeasible: no path inside the window ..." when the
 *              score is -inf; the output is then untouched.
 *   feed_back  needs posteriors and loglik; after rvb_encode, the same batches in DESCENDING order: each must hold exactly the
 *              frames the forward sweep saw at that position, else RVB_E_STATE names what was expected.
 *   finish     RVB_E_STATE unless the backward sweep reached frame 0.  Per token [n_tokens], each nullable, as rvb_ctc_score.
 *   end        releases the buffers.
 * rvb_ctc_align_long_*, the one-batch calls and the search stay usable in between. */
int rvb_ctc_score_long_begin(rvb_engine* e, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states,
                             int posteriors);
int rvb_ctc_score_long_feed(rvb_engine* e);
int rvb_ctc_score_long_loglik(rvb_engine* e, double* loglik);
int rvb_ctc_score_long_feed_back(rvb_engine* e);
int rvb_ctc_score_long_finish(rvb_engine* e, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame);
int rvb_ctc_score_long_end(rvb_engine* e);

/* rvb_ctc_align_wild for a transcript with ALTERNATIVES and OPTIONAL words: each sequence is a left-to-right token GRAPH, and one
 * Viterbi pass (csrc/ctc_graph.hip) picks the reading that was spoken and aligns it.  Sequence i has n_nodes[i] >= 1 nodes in
 * topological order (node_tokens, is_final: concatenated over the sequences).  Node j has a label (a vocab id other than the blank,
 * or RVB_CTC_WILDCARD) and an ordered, duplicate-free predecessor list preds[pred_off[j] .. pred_off[j + 1]) of at least one entry,
 * each a node index < j or -1 for "start"; pred_off holds n_nodes[i] + 1 offsets per sequence (concatenated; the offsets count
 * within the sequence's own predecessors, whose lists are concatenated in `preds`).  At least one node is final and at least one
 * has a start predecessor.  Lattice states: B_start (the leading blank) and per node T_j (emits the label; a wildcard emits
 * w[t] + wildcard_bias as in rvb_ctc_align_wild) and B_j (the blank after it).  Frame 0: B_start, and T_j where -1 is a predecessor.
 * Frame t >= 1, candidates in order, the FIRST maximum wins: B_start: stay; B_j: stay, T_j; T_j: stay, then per predecessor in list
 * order B_pred (B_start for -1), then T_pred if the predecessor is a node of another label (two wildcards are one label).  The path
 * ends in the best of B_f, T_f over the final nodes in ascending order, first maximum.  On a chain (pred[j] = {j - 1}, pred[0] =
 * {-1}, the last node final) every output is bit-identical to rvb_ctc_align_wild's.
 * Outputs (each nullable): labels / frame_node [sum of the sequences' frames]: per frame the label (blank id on a blank) and the
 * node index within the sequence (-1 on a blank); path_len [n_seq] = nodes on the chosen path; path_nodes / begin / end / peak /
 * confidence: per path position, sequence i's starting at its node offset (sum of n_nodes[..i)), as rvb_ctc_align defines them per
 * token; score [n_seq].  Refused by name with sequence and node (RVB_E_ARG), writing nothing: an empty graph, a label outside
 * [0, vocab) that is not the wildcard, a blank label, a predecessor >= j or < -1, a duplicate predecessor, an empty list, no final
 * node, no start predecessor, a bias that is positive or not finite, a chunk range outside the batch, a graph no path of which
 * the frames can emit with a finite score.  Caps per graph (RVB_E_UNSUPPORTED, before any device work;
 * rvb_ctc_align_graph_limits), frames as RVB_CTC_ALIGN_MAX_FRAMES; back-pointers take 1 byte per frame and node of device memory
 * (RVB_E_NOMEM naming the bytes if they do not fit): */
#define RVB_CTC_GRAPH_MAX_NODES 8192        /* every node's scores of two frames live in one workgroup's LDS (128 KiB of 160) */
#define RVB_CTC_GRAPH_MAX_IN_DEGREE 64      /* the winning predecessor's index takes 7 bits of the back-pointer byte */
#define RVB_CTC_GRAPH_MAX_ARCS 32768        /* predecessors of all nodes of one graph */
int rvb_ctc_align_graph(rvb_engine* e, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off,
                        const int32_t* preds, const uint8_t* is_final, int n_seq, const int32_t* first_chunk, const int32_t* n_chunks,
                        float wildcard_bias, int32_t* labels, int32_t* frame_node, int32_t* path_len, int32_t* path_nodes,
                        int32_t* begin, int32_t* end, int32_t* peak, float* confidence, float* score);
int rvb_ctc_align_graph_limits(int32_t* max_nodes, int32_t* max_in_degree, int32_t* max_arcs, int32_t* max_frames);

/* LONG-FORM alignment of a transcript with alternatives: rvb_ctc_align_graph for ONE graph of any number of nodes and arcs over a
 * recording that is encoded in several batches (a WINDOWED graph Viterbi, csrc/ctc_graph_window.hip), by the protocol of
 * rvb_ctc_align_long_*.  Graph, labels, predecessor lists, finals, the states B_start, T_j, B_j, the candidate order and "first
 * maximum wins" are rvb_ctc_align_graph's.  The band is new:
 *   W nodes are alive at a frame: window_nodes, 0 (the default, 8192) or a multiple of 256 in [256, 8192], reduced to the node count
 *   rounded up to 64 when the graph is smaller.  lo_of[t], the window of the launch that computes frame t, is a multiple of 64 and
 *   never decreases; lo_of[0] = 0.  Node j is alive at t iff lo_of[t] <= j < min(lo_of[t] + W, n_nodes); B_start iff lo_of[t] == 0.
 *   A predecessor candidate p -> T_j at frame t counts iff j is alive at t and p >= lo_of[t] (p = -1: iff lo_of[t] == 0); the stay
 *   candidates of an alive node always count.  A node above every window so far holds -inf, one below lo is never read again, a
 *   candidate that does not count is -inf and never wins (the comparison is strict).  The path ends in the best of B_f, T_f over
 *   the final nodes alive at the last frame, ascending, first maximum.
 * With W >= n_nodes rounded up to 64 the window never moves: labels, frame nodes, path and score are rvb_ctc_align_graph's bit for
 * bit, however the batches cut the recording.  Otherwise the result is the best path inside the windows, with an exact fp32 score
 * of its own, and min_margin is that path's smallest distance in nodes to a window edge that is not the graph's own (the lower edge
 * counts where lo_of[t] > 0, the upper where lo_of[t] + W < n_nodes; blank frames count with their node, B_start frames do not; W
 * when no frame counts).  The window follows the best partial path; because an arc may jump over many nodes (the alternatives that
 * were not spoken), a launch lasts only for as long as that path cannot have left through the window's top.
 *   begin   one graph as rvb_ctc_align_graph's (n_nodes + 1 offsets in pred_off); total_frames = the valid encoder frames of ALL
 *           batches to come (<= RVB_CTC_ALIGN_MAX_FRAMES).  Refusals in rvb_ctc_align_graph's words by node, all before any device
 *           work; no node or arc cap, the in-degree cap stays.  Also refused: a bad window_nodes (RVB_E_ARG), a graph whose
 *           shortest reading needs more frames than total_frames (RVB_E_ARG "infeasible"), and, when the window does not hold the
 *           whole graph, an arc whose span j - p exceeds W / 2 - 64, a start predecessor counting as j + 1 (RVB_E_UNSUPPORTED
 *           naming the node and the span: ask for a wider window).  Back-pointers take total_frames x W bytes (RVB_E_NOMEM naming
 *           them).  begin while a lattice is open replaces it.
 *   feed    after rvb_encode, as rvb_ctc_align_long_feed.  RVB_E_STATE before begin, before rvb_encode, or when the batch holds
 *           more frames than the lattice has left.
 *   finish  RVB_E_STATE unless exactly total_frames were fed.  labels / frame_node [total_frames], path_len [1], path_nodes /
 *           begin / end [n_nodes] per path position, score, min_margin (each nullable), as rvb_ctc_align_graph defines them.
 *           RVB_E_ARG "infeasible: no path inside the window ..." when the score is -inf; outputs are then untouched.
 *   end     releases the buffers.
 * Peaks and confidences: encode the batches a second time and pass each its part of finish's labels to
 * rvb_ctc_align_long_emissions, which needs no open lattice.  The one-batch calls, rvb_ctc_align_long_*, rvb_ctc_score_long_* and
 * the search stay usable between begin and finish.  The full sum and the per-node posteriors of such a graph come from
 * rvb_ctc_score_graph_long_* (below), a lattice of its own.  Not offered: several graphs per call. */
int rvb_ctc_align_graph_long_limits(int32_t* max_frames, int32_t* max_in_degree, int32_t* max_window_nodes, int32_t* default_window_nodes);
int rvb_ctc_align_graph_long_begin(rvb_engine* e, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                   const uint8_t* is_final, int64_t total_frames, int window_nodes, float wildcard_bias);
int rvb_ctc_align_graph_long_feed(rvb_engine* e);
int rvb_ctc_align_graph_long_finish(rvb_engine* e, int32_t* labels, int32_t* frame_node, int32_t* path_len, int32_t* path_nodes,
                                    int32_t* begin, int32_t* end, float* score, int32_t* min_margin);
int rvb_ctc_align_graph_long_end(rvb_engine* e);

/* Full-sum CTC score of a KNOWN transcript: log p(tokens | frames) summed over every alignment, the quantity the reference calls
 * the CTC loss (CTC.forward, asr/wenet/transformer/ctc.py:65-104 = torch.nn.CTCLoss(reduction='sum') over
 * log_softmax(ctc_lo(encoder_out)), reported by bin/get_loss.py): loglik = -loss.  Valid after rvb_encode / rvb_stream_finish; the
 * sequences, chunk ranges, refusals (by the same names) and caps are those of rvb_ctc_align, and n_seq > 1 scores several transcripts
 * (or several chunk ranges) in one launch, which is how candidate transcripts are compared.  loglik [n_seq] is fp64: normalised fp32
 * forward variables plus per-frame offsets summed in fp64 (csrc/ctc_forward_backward.hip).  The reference's zero_infinity=True turns
 * a transcript that the frames cannot emit into loss 0; this call does NOT: it refuses (RVB_E_ARG) exactly as rvb_ctc_align does.
 * Per-token outputs (each nullable, concatenated like `tokens`), from the posteriors gamma[t][token] of a backward sweep:
 * occupancy = sum over frames of the posterior (the expected number of frames of the token), mean_frame = the posterior-weighted
 * mean frame, peak_post = the largest posterior, peak_frame = its frame (first on ties).  With all four null only the forward sweep
 * runs and nothing is stored per frame; otherwise the forward sweep keeps its rows, 4 bytes per frame and state (states = 2 tokens + 1
 * padded to a multiple of 32) of device memory: RVB_E_NOMEM naming the byte count if they do not fit. */
int rvb_ctc_score(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* first_chunk,
                  const int32_t* n_chunks, double* loglik, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame);

/* rvb_ctc_score for a transcript with ALTERNATIVES and OPTIONAL words: the full-sum score over a token GRAPH, in one pass
 * (csrc/ctc_graph_score.hip).  Graph, labels, predecessor lists, finals, states and chunk ranges are exactly those of
 * rvb_ctc_align_graph, with log-sum-exp where that call takes the maximum:
 *   frame 0:  a(B_start) = lp[0][blank];  a(T_j) = lp[0][tok_j] if -1 is a predecessor of j, else -inf;  a(B_j) = -inf
 *   frame t:  a(B_start) = a'(B_start) + lp[t][blank];  a(B_j) = lse(a'(B_j), a'(T_j)) + lp[t][blank];
 *             a(T_j) = lse(a'(T_j), per predecessor p: a'(B_p) (a'(B_start) for -1), and a'(T_p) if tok_p != tok_j) + lp[t][tok_j]
 *   loglik  = lse over the final nodes f of a_{T-1}(B_f), a_{T-1}(T_f)
 * so loglik [n_seq] (fp64, normalised as rvb_ctc_score's) = log of the sum over the graph's node paths pi of p_CTC(labels(pi) | frames).
 * Two node paths that spell the same tokens are two paths and both count: the graph {a|a} scores loglik(a) + log 2.  Nothing is
 * deduplicated.
 * Per-node outputs (each nullable, concatenated like node_tokens), from the posteriors gamma_t(T_j) of a backward sweep: occupancy,
 * mean_frame (-1 where the occupancy is exactly 0), peak_post and peak_frame (first on ties) as rvb_ctc_score defines them per token,
 * and visit = the probability that the path passes through node j, i.e. the summed posterior of the readings that contain it
 * (sum over frames of the mass that enters T_j).  With all five null only the forward sweep runs and nothing is stored per frame;
 * otherwise the forward sweep keeps a(T_j) of every frame, 4 bytes per frame and node (nodes padded to a multiple of 64) of device
 * memory: RVB_E_NOMEM naming the byte count if they do not fit.
 * Refusals and caps are those of rvb_ctc_align_graph, in the same words after this call's name, all before any device work and with
 * every output untouched; in addition RVB_CTC_WILDCARD is refused (RVB_E_ARG, naming sequence and node: the maximum over the
 * vocabulary is no probability), a graph whose shortest reading needs more frames than there are is refused as infeasible
 * (RVB_E_ARG), and, only when a per-node output is asked for, a node with more than RVB_CTC_GRAPH_MAX_IN_DEGREE SUCCESSORS
 * (RVB_E_UNSUPPORTED, naming sequence and node).  A graph that the frames cannot emit with a finite score is refused (RVB_E_ARG) after
 * the forward sweep. */
int rvb_ctc_score_graph(rvb_engine* e, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off,
                        const int32_t* preds, const uint8_t* is_final, int n_seq, const int32_t* first_chunk, const int32_t* n_chunks,
                        double* loglik, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame);

/* LONG-FORM full-sum score of a transcript with alternatives: rvb_ctc_score_graph (loglik, and with posteriors the per-node visit,
 * occupancy, mean frame, peak posterior and its frame) for ONE graph of any number of nodes and arcs over a recording that is encoded
 * in several batches (a WINDOWED full sum over the graph, csrc/ctc_graph_fb_window.hip), by the protocol of rvb_ctc_score_long_*.
 * Graph, states, recurrences and the definitions of loglik, the posteriors and visit are rvb_ctc_score_graph's; the states are carried
 * in fp64 as there.  The band is rvb_ctc_align_graph_long_*'s with log-sum-exp in place of the maximum:
 *   W nodes are alive at a frame: window_nodes, 0 (the default, 4096) or a multiple of 256 in [256, 4096] (the fp64 states halve the
 *   aligner's cap), reduced to the node count rounded up to 64.  lo_of[t] is a multiple of 64 and never decreases; lo_of[0] = 0.
 *   Node j is alive at t iff lo_of[t] <= j < min(lo_of[t] + W, n_nodes); B_start iff lo_of[t] == 0.  A transition into T_j at t from
 *   predecessor p counts iff j is alive at t and p >= lo_of[t] (p = -1: iff lo_of[t] == 0); stay transitions of an alive node
 *   always count; a node that was not alive before holds -inf.  loglik is the log-sum over the final nodes alive at the last frame
 *   (<= the full sum of the whole graph), and the posteriors are those of that sum: over the alive states of a frame they add up
 *   to 1, also across a window move.  The window follows the first maximum of the normalised forward row over the states that can
 *   still reach a final end, placed and cut by the aligner's policy.
 * With W >= n_nodes rounded up to 64 the window never moves: loglik and all five per-node outputs are then rvb_ctc_score_graph's bit
 * for bit (for graphs of at most 4096 nodes), however the batches cut the recording.
 *   begin      one graph as rvb_ctc_align_graph_long_begin's; refusals in its words and rvb_ctc_score_graph's (a wildcard; with
 *              posteriors a node with more than 64 successors; the window; the span; the infeasible shortest reading), all before
 *              any device work.  posteriors != 0 keeps the forward rows, total_frames x W x 4 bytes (RVB_E_NOMEM naming them).
 *              begin while a lattice is open replaces it.
 *   feed       after rvb_encode, batches in ASCENDING order.  RVB_E_STATE before begin, before rvb_encode, or when the batch holds
 *              more frames than the lattice has left.
 *   loglik     RVB_E_STATE unless exactly total_frames were fed.  RVB_E_ARG "infeasible: no path inside the window ..." when the
 *              sum is -inf; the output is then untouched.
 *   feed_back  needs posteriors and loglik; after rvb_encode, the same batches in DESCENDING order: each must hold exactly the
 *              frames the forward sweep saw at that position, else RVB_E_STATE names what was expected.
 *   finish     RVB_E_STATE unless the backward sweep reached frame 0.  Per node [n_nodes], each nullable, as rvb_ctc_score_graph.
 *   end        releases the buffers.
 * The one-batch calls, the other long lattices and the search stay usable in between.  Not offered: wildcards in the sum, several
 * graphs per call. */
int rvb_ctc_score_graph_long_limits(int32_t* max_frames, int32_t* max_in_degree, int32_t* max_window_nodes, int32_t* default_window_nodes);
int rvb_ctc_score_graph_long_begin(rvb_engine* e, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                   const uint8_t* is_final, int64_t total_frames, int window_nodes, int posteriors);
int rvb_ctc_score_graph_long_feed(rvb_engine* e);
int rvb_ctc_score_graph_long_loglik(rvb_engine* e, double* loglik);
int rvb_ctc_score_graph_long_feed_back(rvb_engine* e);
int rvb_ctc_score_graph_long_finish(rvb_engine* e, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame);
int rvb_ctc_score_graph_long_end(rvb_engine* e);

/* Phrase search: EVERY occurrence of given short phrases (names, terms) in the audio of the last rvb_encode / rvb_stream_finish, on
 * the device (csrc/ctc_find.hip, one wave per phrase and sequence).  n_phrases phrases, concatenated in `tokens`, tok_lens[p] ids
 * each (1 .. RVB_CTC_FIND_MAX_TOKENS, in [0, vocab), none the blank); n_seq sequences of frames given by first_chunk / n_chunks as
 * for rvb_ctc_align (the VALID frames of the chunks, concatenated, numbered within the sequence), so a hit may straddle a chunk
 * boundary.  Every phrase is searched in every sequence; pair p * n_seq + i is phrase p in sequence i.
 * A phrase is the lattice z = [y0, blank, y1, ..., y(L-1)] with a free start and a free end.  Frame t emits
 * d[t][s] = lp[t][z[s]] - w[t] in fp32, w[t] = the largest log-prob of the frame (what a wildcard frame of rvb_ctc_align_wild
 * costs): d <= 0, and 0 exactly where the model's own greedy label agrees.  h[t][0] = max(h[t-1][0], 0) + d[t][0], the 0 standing for
 * "starts here"; h[t][s] = max(h[t-1][s], h[t-1][s-1] (, h[t-1][s-2] if z[s] is a token other than z[s-2])) + d[t][s], the first
 * maximum in that order (a stay beats a fresh start on a tie), each state carrying the start frame of its chosen path.  Frame t is an
 * ARRIVAL when the last state is entered (not stayed in) at t; an arrival with score h >= threshold[p] (fp32, total nats, <= 0;
 * -inf keeps every arrival) is a CANDIDATE (start, end = t, score).  Per pair the first max_candidates candidates in frame order are
 * kept on the device and then suppressed on the host: by score descending, then end ascending, then start ascending, a candidate
 * is kept if [start, end] meets no kept span, until max_hits are kept; nothing is suppressed across phrases or sequences.
 * Outputs: n_hits [n_phrases * n_seq]; start / end / score [n_phrases * n_seq][max_hits], the pair's hits in order of end (score is
 * the fp32 path score: 0 = the greedy labels spell the phrase; divide by tok_lens[p] to compare phrases); n_candidates (nullable)
 * [n_phrases * n_seq] = all arrivals at or above the threshold, kept or not: a value above max_candidates says that later arrivals
 * were dropped and the call should be repeated with a larger cap.  A sequence with fewer frames than a phrase needs is no error: it
 * has no arrival.  Refused by name before any device work: RVB_E_ARG for an empty phrase, an id outside [0, vocab) or equal to the
 * blank, n_phrases, n_seq, max_candidates or max_hits < 1, a threshold that is NaN or > 0, a chunk range outside the batch;
 * RVB_E_UNSUPPORTED for a phrase of more than RVB_CTC_FIND_MAX_TOKENS tokens (locate longer text with rvb_ctc_align_wild and a
 * wildcard on either side); RVB_E_NOMEM, naming the bytes, if the candidate buffers (12 bytes per pair and candidate) do not fit. */
#define RVB_CTC_FIND_MAX_TOKENS 32
int rvb_ctc_find(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_phrases, const float* threshold /* [n_phrases] */,
                 const int32_t* first_chunk, const int32_t* n_chunks, int n_seq, int max_candidates, int max_hits,
                 int32_t* n_hits /* [n_phrases*n_seq] */, int32_t* start, int32_t* end, float* score /* [n_phrases*n_seq*max_hits] each */,
                 int64_t* n_candidates /* [n_phrases*n_seq], nullable: arrivals above threshold, kept or not */);

/* ctc_prefix_beam_search (search.py:124-248), float64 host arithmetic, one host thread per chunk.
 * Results are kept in the engine; read them with rvb_get_nbest. */
int rvb_ctc_prefix_beam(rvb_engine* e, int beam);
int rvb_get_nbest_count(rvb_engine* e, int chunk, int32_t* n_hyps, int32_t* max_len);
/* Hot-word context biasing of ctc_prefix_beam_search: the ContextGraph of asr/wenet/utils/context_graph.py:103-265 (an Aho-Corasick
 * automaton over token ids) applied as search.py:169-233 does.  n_phrases phrases, concatenated in `tokens`, lens[i] ids each; every
 * matched token of a phrase earns context_score, a broken match gives its bonus back, a completed one keeps it.  The graph never
 * changes which tokens a frame offers (still the top-`beam` of its log-probs): it reorders the host beam, which is pruned by
 * score + context score; the scores rvb_get_nbest reports include the context score each hypothesis ends with.
 * n_phrases == 0 clears the graph.  Empty phrases are allowed and ignored.  RVB_E_ARG, with the phrase and position named: a token
 * id outside [0, vocab) or equal to the blank id, a negative length.  The engine copies what it needs; the graph stays until it is
 * replaced or cleared and applies to every later rvb_ctc_prefix_beam -- after rvb_encode and after rvb_stream_finish alike -- and
 * through its n-best and scores to rvb_attention_rescore (ctc_weight * biased score, search.py:436-444).  rvb_ctc_greedy,
 * rvb_attention_decode and rvb_joint_decode ignore it, as the reference's modes do.  Without a graph the search executes exactly the
 * float64 operations it always did. */
int rvb_set_context_graph(rvb_engine* e, const int32_t* tokens, const int32_t* lens, int n_phrases, double context_score);
/* tokens/times: [n_hyps][max_len] padded with -1; lens/times_lens/scores: [n_hyps] */
int rvb_get_nbest(rvb_engine* e, int chunk, int32_t* tokens, int32_t* lens, int32_t* times, int32_t* times_lens,
                  double* scores);

/* attention_rescoring (search.py:363-448) over the stored n-best of every chunk of the batch.
 * Per chunk: index of the winning hypothesis, its score (fp32 accumulation as the reference),
 * confidence, and per-token confidences [max_len] of the winner. */
/* Optional, between rvb_encode and rvb_ctc_prefix_beam when rvb_attention_rescore will follow: enqueues the decoders' memory
 * key / value projections (decoder_layer.py:112-119 `src_attn(x, memory, memory)`), which depend on the encoder output alone,
 * so that the device computes them while the host searches the last slice.  rvb_attention_rescore does it itself otherwise. */
int rvb_prepare_rescoring(rvb_engine* e, int right_to_left);
int rvb_attention_rescore(rvb_engine* e, double ctc_weight, double reverse_weight);
/* Attention-decoder loss and accuracy of KNOWN transcripts: the teacher-forced pass of ASRModel._calc_att_loss (asr_model.py:248-286)
 * on the chunks of the last rvb_encode / rvb_stream_finish.  n_seq sequences, concatenated in `tokens` (tok_lens[i] ids each);
 * sequence i is scored against the memory of chunk chunk_of[i] -- ONE chunk: its frames are the only memory the decoder path has.
 * Decoder inputs are [sos] + y, targets y + [eos]; the right-to-left decoder (run only when reverse_weight > 0) sees the reversed y
 * (reverse_pad_list + add_sos_eos).  The sequences form the prefix trie of rvb_attention_rescore, so candidates of one chunk share the
 * decoder rows of their common prefix and each one reads the bits it would read alone; the memory keys / values of
 * rvb_prepare_rescoring are reused.  Per sequence: loss_l / loss_r = the label-smoothed KL of LabelSmoothingLoss
 * (label_smoothing_loss.py:68-96, smoothing = lsm_weight) SUMMED over the L + 1 positions, in fp64, divided by nothing (loss_r
 * nullable; zeros when reverse_weight = 0); n_correct = positions of the left decoder whose arg-max equals the target, the <eos>
 * position included (th_accuracy, utils/common.py:268-287; ties to the lowest index); n_positions = L + 1.  The caller forms
 * loss_att = (1 - reverse_weight) loss_l + reverse_weight loss_r, normalised as its configuration says.  Flat per-position outputs,
 * concatenated in sequence order with L + 1 entries each, every one nullable: logp_l, logp_r (in the right decoder's own order:
 * position j is its j-th target) = log p(target), top1_l = the left decoder's arg-max.
 * Refused by name: before rvb_encode, a model without decoder, reverse_weight > 0 without a right-to-left decoder (RVB_E_STATE);
 * an empty sequence, an id outside [0, vocab), chunk_of outside the batch, lsm_weight outside [0, 1) (RVB_E_ARG); L + 1 beyond the
 * positional table (RVB_E_UNSUPPORTED).  The n-best lists, the rescoring results and what a later rvb_attention_rescore returns are
 * left as they are. */
int rvb_attention_score(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* chunk_of,
                        double reverse_weight, double lsm_weight, double* loss_l, double* loss_r, int32_t* n_correct,
                        int32_t* n_positions, float* logp_l, float* logp_r, int32_t* top1_l);
/* `attention` mode (asr/wenet/transformer/search.py:251-360): autoregressive beam search with the left decoder on
 * the chunks of the last rvb_encode; per-hypothesis K/V caches on the device, beam bookkeeping on the host in float32
 * as the reference does.  Runs until every beam ended with <eos> or for encoder-frames steps. */
int rvb_attention_decode(rvb_engine* e, int beam, float length_penalty);
/* best hypothesis of one chunk without <sos>/<eos>; `tokens` needs room for rvb_encoder_frames() entries */
int rvb_get_attention_result(rvb_engine* e, int chunk, int32_t* tokens, int32_t* n_tokens, float* score);

/* `joint_decoding` mode (asr/wenet/transformer/search.py:450-496 -> espnet/beam_search_timesync.py:86-508): time-synchronous
 * joint CTC / attention beam search on the chunks of the last rvb_encode, which must have kept at least
 * int(pre_beam_ratio * beam) log-probs per frame.  Every chunk advances one encoder frame per iteration; the prefixes of all
 * chunks that need the attention decoder form one batched decoder step.  The decoder's memory is the chunk's
 * valid frames as a (1, len, d) tensor -- the shape BeamSearchTimeSync.reset expects; the reference's own call passes a 2-D
 * tensor and raises there.  length_bonus is what ASRModel.decode passes as `length_penalty` (asr_model.py:427-431).
 * Result per chunk: winner without <sos>, start / end frame and confidence (max of CTC and attention) per token, joint score. */
int rvb_joint_decode(rvb_engine* e, int beam, double ctc_weight, double pre_beam_ratio, double length_bonus);
int rvb_get_joint_result(rvb_engine* e, int chunk, int32_t* tokens, int32_t* times, int32_t* end_times, double* tokens_confidence,
                         int32_t* n_tokens, double* score);
int rvb_get_joint_stats(rvb_engine* e, int64_t* decoder_rows, int64_t* steps);

int rvb_get_rescored(rvb_engine* e, int chunk, int32_t* best_index, float* score, double* confidence,
                     double* tokens_confidence /* [len of best] */);
/* all chunks of the batch at once: the winning hypothesis of each chunk, arrays padded to [B][T]
 * (T = rvb_encoder_frames) with -1 / 0 */
int rvb_get_rescored_batch(rvb_engine* e, int32_t* lens, int32_t* tokens, int32_t* times_lens, int32_t* times,
                           float* scores, double* confidences, double* tokens_confidence);
/* fp8 engines: forget the activation scales; the next rvb_encode calibrates again (in bf16) on its batch */
int rvb_fp8_recalibrate(rvb_engine* e);
/* fp8 engines: the calibrated per-tensor activation scales, 7 per conformer block (inputs of macaron FFN 1 / its hidden /
 * qkv / pointwise conv 1 / pointwise conv 2 / FFN 1 / its hidden; powers of two, value = fp8 * scale), followed by ONE more entry:
 * the scale of conv1's fp8 output (policy bit 5; 0 = not measured, conv2 then runs in bf16) -- n = 7 * blocks + 1 (round 5: until
 * then the subsampling scale was not part of the vector and ranks of a sharded run could not agree on it).  get: *n = 0 while the
 * engine is not calibrated; `scales` may be NULL to query n.  set: n = 7 * blocks (subsampling scale untouched) or 7 * blocks + 1;
 * installs scales and ends calibration, so that the very next
 * rvb_encode already runs in fp8 -- how the ranks of a sharded run agree on one set (element-wise maximum of what each rank
 * calibrated on its own slice, reverb_amd/dist.py), and how a deployment pins scales measured once. */
int rvb_get_fp8_scales(rvb_engine* e, float* scales, int32_t* n);
/* How many values did NOT fit e4m3 at the installed scales since they were calibrated / installed / last reset: the kernels that
 * write an fp8 operand (the LayerNorms in front of the fp8 GEMMs, the feed-forward's fp8 epilogue) clip to +-448 and count what they
 * clip, per block and activation slot in the order of rvb_get_fp8_scales (n = 7 * blocks; counts may be NULL to query n).
 * A calibrated engine decoding audio like its calibration batch reports zeros (2x headroom); anything else says the scales do
 * not cover this input -- recalibrate (rvb_fp8_recalibrate) or install wider scales.  reset != 0 zeroes the counters. */
int rvb_get_fp8_saturation(rvb_engine* e, uint32_t* counts, int32_t* n, int reset);
/* Round 4: rvb_set_fp8_policy's bit 5 puts the subsampling's second convolution (K = 9 d, a quarter of the encoder's FLOPs;
 * subsampling.py:189-190) on the fp8 path: conv1 then writes its ReLU output in e4m3 at a scale calibrated with the others.
 * *scale: that scale (0 while not calibrated -- conv2 then stays bf16; the last entry of rvb_get / rvb_set_fp8_scales); *clipped: values of conv1's output beyond 448 * scale since the last reset.  Either may be NULL. */
int rvb_get_fp8_subsample(rvb_engine* e, float* scale, uint32_t* clipped, int reset);
int rvb_set_fp8_scales(rvb_engine* e, const float* scales, int32_t n);
/* Work of the last rvb_attention_rescore: `pairs` = (hypothesis, position) log-probs served = the rows the reference's
 * padded [N, L] decoder batch computes (search.py:391-412); `decoder_rows` = rows actually computed: one per DISTINCT
 * hypothesis prefix of a chunk (the decoder is causal, so hypotheses of one beam share the rows of their common prefix). */
int rvb_get_rescore_stats(rvb_engine* e, int64_t* decoder_rows, int64_t* pairs);
/* per-hypothesis decoder log-probs of the last rescoring (parity tap): for hyp i of `chunk`,
 * out[j] = log p(w_j | ...) for j < len and out[len] = log p(eos); right=1 for the r2l decoder */
int rvb_get_rescore_logp(rvb_engine* e, int chunk, int hyp, int right, float* out);

/* Collectives of the chunk-sharded path (no data-path collective, ONE all-gather of the packed per-chunk results).
 * RCCL is bound directly (resolved with dlopen on first use; PyTorch is not needed): one rank calls rvb_comm_unique_id and
 * hands the 128 bytes to the others by any side channel, every rank calls rvb_comm_init on its engine (one engine = one GPU =
 * one rank), rvb_allgather_results gathers `bytes` bytes per rank (host buffers; recv = world * bytes) in rank order on the
 * engine's stream.  rvb_comm_create / rvb_comm_allgather / rvb_comm_free are the same collective on a stand-alone
 * communicator (own stream; one per process = per GPU), which the ASR results and the diarization shard's classes / embeddings
 * both travel on: reverb_amd/dist.py (`RvbComm`, default_comm) uses it whenever the ranks run on GPUs; torch.distributed only
 * carries the 128-byte id once (or a file does: RvbComm.from_file) and serves the gloo CPU tests. */
typedef struct rvb_comm rvb_comm;
int rvb_comm_unique_id(void* id128 /* out: 128 bytes */);
int rvb_comm_create(int device, int world, int rank, const void* id128, rvb_comm** out);
int rvb_comm_allgather(rvb_comm* c, const void* send, int64_t bytes, void* recv);
/* The collective alone (device to device, HIP events on the communicator's stream, checked): average milliseconds of one
 * all-gather of `bytes` bytes per rank -- the xGMI datapoint of SURVEY 8(e) for the top-beam posterior exchange. */
int rvb_comm_time_allgather(rvb_comm* c, int64_t bytes, int iters, double* avg_ms);
/* Failure handling (the reference has none: it is single-process).  With a timeout set, a collective that
 * does not complete in `seconds` -- a peer died or hangs -- returns RVB_E_TIMEOUT instead of blocking for ever; the
 * communicator is aborted (ncclCommAbort) and every later call on it returns RVB_E_STATE.  The host then exchanges through
 * its rendezvous channel and re-queues the missing rank's chunk range (reverb_amd/dist.py: decode_sharded).  0 = wait for ever. */
int rvb_comm_set_timeout(rvb_comm* c, double seconds);
/* What a launcher needs of a process group besides the gather: a barrier and the maximum of a double over the ranks
 * (bench.py's step timing) -- 8-byte all-gathers on the same communicator, so a rank holds ONE RCCL communicator. */
int rvb_comm_barrier(rvb_comm* c);
int rvb_comm_max_f64(rvb_comm* c, double* value /* in: this rank's, out: the maximum */);
/* The alternative exchange of SURVEY.md 8(e) -- top-beam CTC posteriors instead of decoded results -- device to device: the
 * [B, T, k] fp32 log-probs and int32 ids of the engine's last rvb_encode are gathered straight out of HBM into the
 * communicator's device buffer ([world][vals] then [world][ids]); host_out (nullable, 2 * world * B*T*k*4 bytes) receives a
 * copy; *bytes_per_rank = B*T*k*8.  Every rank must hold the same batch shape. */
int rvb_comm_allgather_topk(rvb_comm* c, rvb_engine* e, void* host_out, int64_t* bytes_per_rank);
int rvb_comm_free(rvb_comm* c);
int rvb_comm_init(rvb_engine* e, int world, int rank, const void* id128);
int rvb_allgather_results(rvb_engine* e, const void* send, int64_t bytes, void* recv);
int rvb_comm_destroy(rvb_engine* e);

/* Stage timing (HIP events on the engine stream).  level 1: every kernel family is bracketed;
 * names: "fbank","subsample","gemm","attention","rownorm","glu_dwconv","ctc_topk","embed",
 * "lse_gather" (the row kernel after the decoders' output layer: rescoring and rvb_attention_score),"search_host","ctc_align_lp" (rvb_ctc_align: CTC head + log-softmax),"ctc_viterbi" (its
 * forward pass + back-trace),"ctc_viterbi_window" (rvb_ctc_align_long_feed / _finish: the windowed launches with their readbacks + back-trace),"ctc_fb_window_forward" / "ctc_fb_window_backward" (rvb_ctc_score_long_*: the two windowed sweeps with their readbacks),"ctc_forward" / "ctc_backward" (rvb_ctc_score: the two sweeps),"ctc_graph_forward" / "ctc_graph_backward" (rvb_ctc_score_graph: the two sweeps),"ctc_graph_fb_window_forward" / "ctc_graph_fb_window_backward" (rvb_ctc_score_graph_long_*: the two windowed sweeps with their readbacks),"ctc_find" (rvb_ctc_find: the search kernel),"ctc_graph" (rvb_ctc_align_graph:
 * forward pass + back-trace).  level 2: only the GEMM launches (the dominant kernel; half the
 * events, ~1 % less perturbation of the step).  level 0: off.
 * flops: algorithmic FLOPs launched (gemm/attention only). */
int rvb_set_profiling(rvb_engine* e, int level);
int rvb_reset_timings(rvb_engine* e);
int rvb_get_timing(rvb_engine* e, const char* name, double* ms, double* flops, int64_t* launches);
/* ALGORITHMIC HBM bytes launched under `name` since the last reset ("gemm" / "gemm_fp8" only): every operand of a GEMM once --
 * A (the NHWC activation once for the implicit convolution), W, bias, C, the fp32 residual.  What `roofline.traffic` (PMC) is
 * compared with. */
int rvb_get_timing_bytes(rvb_engine* e, const char* name, double* bytes);

/* Word error counts of a hypothesis against a reference, both as word-id sequences (host code, no GPU): minimal Levenshtein
 * alignment, counts = {errors, substitutions, deletions, insertions} -- the numbers `fstalign wer` logs as bestWER and
 * asr/wer_evaluation/aggregate_scoring.py:37-44 sums (reverb_amd/wer_evaluation/align.py is the caller). */
int rvb_wer_counts(const int32_t* ref, int64_t n_ref, const int32_t* hyp, int64_t n_hyp, int64_t* counts /* [4] */);

#ifdef __cplusplus
}
#endif
#endif /* RVB_H_ */
