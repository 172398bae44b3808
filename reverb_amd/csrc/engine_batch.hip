// librvb engine: several recordings resident together (rvb_batch_plan, rvb_upload_batch, rvb_batch_n_samples, rvb_fbank_batch).
// The reference decodes a data set in batches through the same model.decode (asr/wenet/bin/recognize.py); here N recordings cost one
// upload call, one fbank launch and ceil(chunks / max_chunks) rvb_encode calls, and every recording keeps the frames, the chunking
// and the zero padding it has when it is uploaded alone (cli/reverb.py:148-180), so its chunks encode to the same bits.
#include "engine_impl.h"

#include <algorithm>
#include <map>

using namespace rvb;

namespace {

constexpr int MAX_BATCH_REC = 65536;

// ceil(new * n / orig) of torchaudio.transforms.Resample(rate, 16000), as resample_uploaded computes it
int64_t len_16k(int64_t n, int rate) {
  if (rate == 16000) return n;
  int a = rate, b = 16000;
  while (b) { const int t = a % b; a = b; b = t; }
  const int64_t orig = rate / a, nw = 16000 / a;
  return (nw * n + orig - 1) / orig;
}

int check_n_rec(const char* who, int n_rec) {
  if (n_rec <= 0) { set_error(std::string(who) + ": n_rec must be at least 1"); return E_ARG; }
  if (n_rec > MAX_BATCH_REC) {
    set_error(std::string(who) + ": " + std::to_string(n_rec) + " recordings in one batch, the cap is " + std::to_string(MAX_BATCH_REC));
    return E_UNSUPPORTED;
  }
  return OK;
}

// frames per recording, first chunk row per recording (+ the total), valid frames per chunk (lens may be null)
void plan(const int64_t* n_samples, int n_rec, int chunk_size, int64_t* n_frames, int64_t* first_chunk, int32_t* lens) {
  int64_t c = 0;
  for (int r = 0; r < n_rec; ++r) {
    const int64_t nf = rvb_num_frames(n_samples[r]);
    const int64_t nc = (nf + chunk_size - 1) / chunk_size;
    if (n_frames) n_frames[r] = nf;
    first_chunk[r] = c;
    if (lens)
      for (int64_t k = 0; k < nc; ++k) lens[c + k] = (int32_t)std::min<int64_t>(chunk_size, nf - k * chunk_size);
    c += nc;
  }
  first_chunk[n_rec] = c;
}

}  // namespace

extern "C" {

int rvb_batch_plan(const int64_t* n_samples, int n_rec, int chunk_size, int64_t* n_frames, int64_t* first_chunk, int32_t* lens) {
  RVB_TRY(check_n_rec("rvb_batch_plan", n_rec));
  if (!n_samples || !n_frames || !first_chunk) { set_error("rvb_batch_plan: null argument (n_samples, n_frames and first_chunk are needed)"); return E_ARG; }
  if (chunk_size < 7) { set_error("rvb_batch_plan: chunk_size must be at least 7 frames"); return E_ARG; }
  for (int r = 0; r < n_rec; ++r)
    if (n_samples[r] < 0) { set_error("rvb_batch_plan: recording " + std::to_string(r) + " has a negative length"); return E_ARG; }
  plan(n_samples, n_rec, chunk_size, n_frames, first_chunk, lens);
  return OK;
}

int rvb_upload_batch(rvb_engine* e, const void* const* data, const int32_t* sample_format, const int64_t* n_samples,
                     const int32_t* sample_rate, int n_rec) {
  // every refusal of an argument comes before the engine is touched
  RVB_TRY(check_n_rec("rvb_upload_batch", n_rec));
  if (!data || !sample_format || !n_samples || !sample_rate) { set_error("rvb_upload_batch: null argument"); return E_ARG; }
  for (int r = 0; r < n_rec; ++r) {
    const std::string who = "rvb_upload_batch: recording " + std::to_string(r);
    if (sample_format[r] != RVB_SAMPLE_I16 && sample_format[r] != RVB_SAMPLE_F32) {
      set_error(who + " has sample_format " + std::to_string(sample_format[r]) + " (RVB_SAMPLE_I16 or RVB_SAMPLE_F32 are taken)"); return E_ARG;
    }
    if (n_samples[r] < 0) { set_error(who + " has a negative length"); return E_ARG; }
    if (sample_rate[r] < 1000 || sample_rate[r] > 384000) {
      set_error(who + " has sample_rate " + std::to_string(sample_rate[r]) + " (1000 .. 384000 are taken)"); return E_ARG;
    }
    if (!data[r] && n_samples[r] > 0) { set_error(who + " has samples but a null pointer"); return E_ARG; }
  }
  if (!e) { set_error("rvb_upload_batch: null engine"); return E_ARG; }
  if (e->pcm_pending) {
    set_error("rvb_upload_batch: an rvb_upload_pcm_async upload is pending: rvb_fbank consumes it, or a synchronous upload replaces it");
    return E_STATE;
  }
  RVB_HIP_CHECK(hipSetDevice(e->device));

  // layout: every int16 recording's samples packed in e->pcm (read by the fbank at 16 kHz, by the resampler otherwise), float
  // recordings at another rate packed in e->wave_in, float recordings at 16 kHz and every resampler output packed in e->wave_f32
  std::vector<int64_t> in_off(n_rec), n16(n_rec), src(n_rec);
  std::vector<int32_t> is_float(n_rec);
  int64_t n_i16 = 0, n_fin = 0, n_f16 = 0;
  for (int r = 0; r < n_rec; ++r) {
    const bool f32 = sample_format[r] == RVB_SAMPLE_F32, at16 = sample_rate[r] == 16000;
    n16[r] = len_16k(n_samples[r], sample_rate[r]);
    is_float[r] = (f32 || !at16) ? 1 : 0;
    if (!f32) { in_off[r] = n_i16; n_i16 += n_samples[r]; }
    else if (!at16) { in_off[r] = n_fin; n_fin += n_samples[r]; }
    if (is_float[r]) { src[r] = n_f16; n_f16 += n16[r]; }
    else src[r] = in_off[r];
  }
  e->batch = false;                     // whatever fails below leaves no half-made batch behind
  e->packed = false; e->feat_kind = 0;  // ... and no features of an earlier upload (rvb_pause_chunks)
  RVB_TRY(e->pcm.ensure((size_t)n_i16 * 2 + 16));
  RVB_TRY(e->wave_in.ensure((size_t)std::max<int64_t>(n_fin, 1) * 4));
  RVB_TRY(e->wave_f32.ensure((size_t)std::max<int64_t>(n_f16, 1) * 4));

  // the resampling taps of every rate of the batch, in one device buffer
  struct Taps { size_t off; int orig, nw, width, K; };
  std::map<int, Taps> taps;
  std::vector<float> all_taps;
  for (int r = 0; r < n_rec; ++r) {
    if (sample_rate[r] == 16000 || taps.count(sample_rate[r])) continue;
    std::vector<float> ker;
    Taps t{all_taps.size(), 0, 0, 0, 0};
    resample_taps(sample_rate[r], 16000, &ker, &t.orig, &t.nw, &t.width, &t.K);
    all_taps.insert(all_taps.end(), ker.begin(), ker.end());
    taps[sample_rate[r]] = t;
  }
  if (!all_taps.empty()) {
    RVB_TRY(e->rs_kernel.ensure(all_taps.size() * 4));
    RVB_HIP_CHECK(hipMemcpyAsync(e->rs_kernel.p, all_taps.data(), all_taps.size() * 4, hipMemcpyHostToDevice, e->stream));
  }
  for (int r = 0; r < n_rec; ++r) {
    const int64_t n = n_samples[r];
    if (n == 0) continue;
    const bool f32 = sample_format[r] == RVB_SAMPLE_F32, at16 = sample_rate[r] == 16000;
    void* dst = !f32 ? (void*)(e->pcm.as<int16_t>() + in_off[r])
                     : at16 ? (void*)(e->wave_f32.as<float>() + src[r]) : (void*)(e->wave_in.as<float>() + in_off[r]);
    RVB_HIP_CHECK(hipMemcpyAsync(dst, data[r], (size_t)n * (f32 ? 4 : 2), hipMemcpyHostToDevice, e->stream));
    if (at16) continue;
    const Taps& t = taps[sample_rate[r]];
    const float* ker = e->rs_kernel.as<float>() + t.off;
    float* out = e->wave_f32.as<float>() + src[r];
    Scope sc(e, "resample");
    if (f32) RVB_TRY(resample_f32(e->stream, e->wave_in.as<float>() + in_off[r], n, ker, t.orig, t.nw, t.width, t.K, out, n16[r]));
    else RVB_TRY(resample(e->stream, e->pcm.as<int16_t>() + in_off[r], n, ker, t.orig, t.nw, t.width, t.K, out, n16[r]));
  }
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));       // the caller's buffers and the taps are free from here on
  e->batch_n = std::move(n16);
  e->batch_src = std::move(src);
  e->batch_is_float = std::move(is_float);
  e->n_samples = 0; e->n_frames = 0; e->feat_rows = 0;
  e->batch = true;
  return OK;
}

int rvb_batch_n_samples(rvb_engine* e, int64_t* out) {
  if (!e || !out) { set_error("rvb_batch_n_samples: null argument"); return E_ARG; }
  if (!e->batch) { set_error("rvb_batch_n_samples: no batch of recordings: call rvb_upload_batch first"); return E_STATE; }
  std::copy(e->batch_n.begin(), e->batch_n.end(), out);
  return OK;
}

int rvb_fbank_batch(rvb_engine* e, int chunk_size, float* feats_out, int64_t* n_frames, int64_t* first_chunk) {
  if (chunk_size < 7) { set_error("rvb_fbank_batch: chunk_size must be at least 7 frames"); return E_ARG; }
  if (!e || !n_frames || !first_chunk) { set_error("rvb_fbank_batch: null argument (the engine, n_frames and first_chunk are needed)"); return E_ARG; }
  if (chunk_size > e->cfg.chunk_frames) {
    set_error("rvb_fbank_batch: chunk_size " + std::to_string(chunk_size) + " exceeds the engine's chunk_frames " + std::to_string(e->cfg.chunk_frames));
    return E_ARG;
  }
  if (!e->fb_window.p) { set_error("rvb_fbank_batch before rvb_finalize"); return E_STATE; }
  if (!e->batch) { set_error("rvb_fbank_batch: no batch of recordings: call rvb_upload_batch first (rvb_fbank serves a single upload)"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  e->packed = false; e->feat_kind = 0;  // rvb_pause_chunks: an fbank call restores the fixed layout
  const int n_rec = (int)e->batch_n.size();
  plan(e->batch_n.data(), n_rec, chunk_size, n_frames, first_chunk, nullptr);
  e->h_frame0.resize(n_rec + 1);
  e->h_rec.resize(n_rec);
  int64_t f = 0;
  for (int r = 0; r < n_rec; ++r) {
    e->h_frame0[r] = f;
    e->h_rec[r] = FbankRec{e->batch_src[r], first_chunk[r] * chunk_size, e->batch_is_float[r], 0};
    f += n_frames[r];
  }
  e->h_frame0[n_rec] = f;
  const int64_t rows = first_chunk[n_rec] * chunk_size;
  RVB_TRY(e->feats.ensure((size_t)std::max<int64_t>(rows, 1) * 80 * 4));
  RVB_TRY(e->d_frame0.ensure(e->h_frame0.size() * 8));
  RVB_TRY(e->d_rec.ensure(e->h_rec.size() * sizeof(FbankRec)));
  RVB_HIP_CHECK(hipMemcpyAsync(e->d_frame0.p, e->h_frame0.data(), e->h_frame0.size() * 8, hipMemcpyHostToDevice, e->stream));
  RVB_HIP_CHECK(hipMemcpyAsync(e->d_rec.p, e->h_rec.data(), e->h_rec.size() * sizeof(FbankRec), hipMemcpyHostToDevice, e->stream));
  FbankTables t{e->fb_window.as<float>(), e->fb_twiddle.as<float>(), e->fb_melw.as<float>(), e->fb_lo.as<int>(), e->fb_hi.as<int>()};
  {
    Scope sc(e, "fbank");
    RVB_TRY(fbank_batch(e->stream, e->pcm.as<int16_t>(), e->wave_f32.as<float>(), e->d_frame0.as<int64_t>(), e->d_rec.as<FbankRec>(), n_rec,
                        f, e->feats.as<float>(), rows, t));
  }
  if (e->copy_stream) RVB_HIP_CHECK(hipEventRecord(e->pcm_free, e->stream));     // the PCM buffers are idle from here on
  if (feats_out && rows) {
    RVB_HIP_CHECK(hipMemcpyAsync(feats_out, e->feats.p, (size_t)rows * 80 * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  e->n_frames = f; e->feat_rows = rows; e->feat_kind = 2;
  return OK;
}

}  // extern "C"
