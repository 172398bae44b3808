// librvb engine: weight packing, workspace and the encode / search / rescore pipeline.
// Orchestrates the kernels of gemm.hip, attention.hip, elementwise.hip, fbank.hip so that one call
// processes a whole batch of 20.51 s chunks (the reference loops chunk by chunk with batch 1,
// asr/wenet/cli/reverb.py:220-253).  Reference structure followed per stage is cited inline.
// This file: the error text, device buffers, profiling, uploads, the GEMM / norm wrappers and the C ABI of include/rvb.h.  The stages
// are engine_weights.hip, engine_encode.hip, engine_decode.hip (with rvb_attention_score) and engine_ctc.hip (with the rvb_ctc_*
// lattice entry points); engine_impl.h declares what they share.
#include "engine_impl.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace rvb {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }

int DevBuf::ensure(size_t n) {
  if (n <= bytes && p) return OK;
  if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
  if (n == 0) n = 16;
  hipError_t err = hipMalloc(&p, n);
  if (err != hipSuccess) {
    p = nullptr;
    (void)hipGetLastError();      // HIP's thread-local last error is sticky: a caller that retries with a smaller size must not
                                  // trip over this failure at its next hipGetLastError() check
    set_error("hipMalloc of " + std::to_string(n) + " bytes failed: " + hipGetErrorString(err));
    return E_NOMEM;
  }
  bytes = n;
  return OK;
}
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }

// ------------------------------------------------------------------------------------ profiling
static void drain_prof(rvb_engine* e) {
  if (e->pending.empty()) return;
  (void)hipStreamSynchronize(e->stream);
  for (auto& p : e->pending) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p.a, p.b);
    e->prof[p.name].ms += ms;
    e->event_pool.push_back(p.a); e->event_pool.push_back(p.b);
  }
  e->pending.clear();
}

// ------------------------------------------------------------------------------------ helpers
int upload_f32(rvb_engine* e, DevBuf& dst, const float* src, size_t n) {
  RVB_TRY(dst.ensure(n * 4));
  RVB_HIP_CHECK(hipMemcpyAsync(dst.p, src, n * 4, hipMemcpyHostToDevice, e->stream));
  return OK;
}
int upload_i32(rvb_engine* e, DevBuf& dst, const int32_t* src, size_t n) {
  RVB_TRY(dst.ensure(n * 4 + 16));
  if (n) RVB_HIP_CHECK(hipMemcpyAsync(dst.p, src, n * 4, hipMemcpyHostToDevice, e->stream));
  return OK;
}

// ------------------------------------------------------------------------------------ gemm wrapper
// every attention launch of the engine carries the lab build's RVB_ATTN_* switches (AttnArgs::lab; the product build: none)
const AttnArgs& with_lab(AttnArgs& a) { attention_lab_switches(a); return a; }

// saturation counters of the fp8 activations: one row of 8 per block (+ a guard row: the last block's norm_final names "the next
// block"); zeroed whenever scales are (re)calibrated or installed
int reset_f8sat(rvb_engine* e) {
  static const int on = lab_env("RVB_FP8_SAT") ? atoi(lab_env("RVB_FP8_SAT")) : 1;       // 0: no counters (A/B of their cost)
  if (!on) return OK;
  RVB_TRY(e->d_f8sat.ensure((e->enc.size() + 1) * 8 * 4));
  RVB_HIP_CHECK(hipMemsetAsync(e->d_f8sat.p, 0, (e->enc.size() + 1) * 8 * 4, e->stream));
  return OK;
}

// ALGORITHMIC HBM bytes of one GEMM launch: every operand once -- A [M,K] (the NHWC activation once for the implicit
// convolution, not its 9-fold gather), W [N,K], bias, C [M,N] written once, the fp32 residual read once
double gemm_alg_bytes(const rvb_engine* e, const GemmArgs& g) {
  const double es = g.in_fp8 ? 1.0 : (double)dt_size(e->dtype);
  const double a = g.conv ? (double)(g.M / (g.cT2 * g.cF2)) * g.cT1 * g.cF1 * g.cC * es : (double)g.M * g.K * es;
  const double c = (double)g.M * (g.act == ACT_GLU ? g.N / 2 : g.N) * (g.out_fp8 ? 1.0 : (g.out_f32 ? 4.0 : (double)dt_size(e->dtype)));
  return a + (double)g.N * g.K * es + (g.bias ? 4.0 * g.N : 0.0) + c + (g.res ? 4.0 * (double)g.M * g.N : 0.0);
}

int run_gemm(rvb_engine* e, const void* A, int lda, const Linear& L, void* C, int ldc, int M, bool out_f32, float alpha,
             int act, const float* res, int ldres) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.W = L.w.p; g.bias = L.b.as<float>(); g.res = res; g.C = C;
  g.M = M; g.N = L.out; g.K = L.in; g.lda = lda; g.ldw = L.in; g.ldc = ldc; g.ldres = ldres;
  g.alpha = alpha; g.act = act; g.out_f32 = out_f32 ? 1 : 0;
  Scope sc(e, "gemm", 2.0 * M * (double)L.out * L.in, gemm_alg_bytes(e, g));
  const int rc = gemm(e->stream, e->dtype, g);
  tap_note_gemm(e);
  return rc;
}
// ---- encoder taps (rvb_set_encoder_tap): with the switch off, or outside the tapped position, neither does anything
int tap_keep(rvb_engine* e, const char* name, const void* src, size_t elems, bool is_bf16) {
  if (!e->tap_live) return OK;
  auto& t = e->taps[name];
  const size_t bytes = elems * (is_bf16 ? 2 : 4);
  RVB_TRY(t.buf.ensure(bytes));
  t.elems = elems; t.bf16 = is_bf16;
  RVB_HIP_CHECK(hipMemcpyAsync(t.buf.p, src, bytes, hipMemcpyDeviceToDevice, e->stream));
  return OK;
}
void tap_note_gemm(rvb_engine* e) {
  if (e->tap_live) e->tap_forms.push_back((float)gemm_last_path());       // what gemm() itself reports of the call just made
}
void tap_note_attention(rvb_engine* e) {
  if (!e->tap_live) return;
  const AttnForm f = attention_last_form(false);
  for (int v : {f.elem_size, f.dkp, f.has_pos, f.nw, f.fold, f.padk, f.occ, f.mf}) e->tap_forms.push_back((float)v);
}
// out8 / out2_8 > 0: that output is fp8 bytes of value / scale (the calibrated per-tensor scale of the GEMM that reads it)
int run_norm(rvb_engine* e, const float* x, const LNorm& n, void* out, bool out_f32, int M, int d, int mode,
             int silu, const void* add, const LNorm* second, void* out2, float out8, float out2_8, bool x_bf16, unsigned* sat,
             unsigned* sat2) {
  NormArgs a;
  a.sat = sat; a.sat2 = sat2;
  a.x_bf16 = x_bf16 ? 1 : 0;
  a.x = x; a.gamma = n.g.as<float>(); a.beta = n.b.as<float>(); a.eps = n.eps; a.mode = mode; a.silu = silu;
  a.add = add; a.out = out; a.out_f32 = out_f32 ? 1 : 0; a.M = M; a.d = d;
  if (second) { a.gamma2 = second->g.as<float>(); a.beta2 = second->b.as<float>(); a.eps2 = second->eps; a.out2 = out2; }
  if (out8 > 0.f) { a.out_fp8 = 1; a.out_inv_scale = 1.f / out8; }
  if (out2_8 > 0.f) { a.out2_fp8 = 1; a.out2_inv_scale = 1.f / out2_8; }
  Scope sc(e, "rownorm");
  return rownorm(e->stream, e->dtype, a);
}
// fp8 GEMM: A8 [M, lda] bytes (values / a_scale), L.w8 / L.wscale; out_kind 0 = compute dtype, 1 = fp32, 2 = fp8 (/ out_scale)
int run_gemm8(rvb_engine* e, const void* A8, int lda, const Linear& L, void* C, int ldc, int M, float a_scale, int out_kind,
              float out_scale, float alpha, int act, const float* res, int ldres, unsigned* sat) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.sat = sat;
  g.A = A8; g.W = L.w8.p; g.bias = L.b.as<float>(); g.res = res; g.C = C;
  g.M = M; g.N = L.out; g.K = L.in; g.lda = lda; g.ldw = L.in; g.ldc = ldc; g.ldres = ldres;
  g.alpha = alpha; g.act = act; g.out_f32 = out_kind == 1; g.out_fp8 = out_kind == 2; g.in_fp8 = 1;
  g.a_scale = a_scale; g.w_scale = L.wscale.as<float>(); g.out_inv_scale = 1.f / out_scale;
  if (!L.w8.p) { set_error("fp8 GEMM on a layer without fp8 weights"); return E_STATE; }
  Scope sc(e, "gemm_fp8", 2.0 * M * (double)L.out * L.in, gemm_alg_bytes(e, g));
  return gemm(e->stream, e->dtype, g);
}

void attention_lab_switches(AttnArgs& a) {
  static const int sw[2] = {
      (lab_env("RVB_ATTN_OCC") && atoi(lab_env("RVB_ATTN_OCC")) == 3 ? ATTN_LAB_OCC3 : 0) |
          (lab_env("RVB_ATTN_MF") && atoi(lab_env("RVB_ATTN_MF")) == 0 ? ATTN_LAB_MF1 : 0) |
          (lab_env("RVB_ATTN_PADK") && atoi(lab_env("RVB_ATTN_PADK")) == 16 ? ATTN_LAB_PADK16 : 0),
      lab_env("RVB_ATTN_PLAIN") ? atoi(lab_env("RVB_ATTN_PLAIN")) : 0};
  a.lab |= sw[0];
  if (sw[1]) a.plain_order = 1;
}

// a synchronous upload replaces whatever rvb_upload_pcm_async left pending (the later call wins)
static int drop_pending_upload(rvb_engine* e) {
  if (e->pcm_pending) {
    RVB_HIP_CHECK(hipStreamSynchronize(e->copy_stream));
    e->pcm_pending = false;
  }
  return OK;
}

// torchaudio.transforms.Resample(sample_rate, 16000) of the uploaded samples (int16 in e->pcm or float in e->wave_in)
// into e->wave_f32 (cli/reverb.py:131-134)
static int resample_uploaded(rvb_engine* e, bool src_float, int64_t n, int sample_rate) {
  const int target = 16000;
  std::vector<float> ker;
  int orig, nw, width, K;
  resample_taps(sample_rate, target, &ker, &orig, &nw, &width, &K);
  const int64_t n_out = (nw * n + orig - 1) / orig;          // ceil(new * length / orig)
  RVB_TRY(e->rs_kernel.ensure(ker.size() * 4));
  RVB_TRY(e->wave_f32.ensure((size_t)std::max<int64_t>(n_out, 1) * 4));
  RVB_HIP_CHECK(hipMemcpyAsync(e->rs_kernel.p, ker.data(), ker.size() * 4, hipMemcpyHostToDevice, e->stream));
  {
    Scope sc(e, "resample");
    if (src_float) RVB_TRY(resample_f32(e->stream, e->wave_in.as<float>(), n, e->rs_kernel.as<float>(), orig, nw, width, K, e->wave_f32.as<float>(), n_out));
    else RVB_TRY(resample(e->stream, e->pcm.as<int16_t>(), n, e->rs_kernel.as<float>(), orig, nw, width, K, e->wave_f32.as<float>(), n_out));
  }
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->n_samples = n_out;
  e->pcm_is_float = true;
  e->batch = false;
  return OK;
}

static void fill_nbest(const PrefixResult& pr, int ml, int32_t* tokens, int32_t* lens, int32_t* times, int32_t* times_lens, double* scores) {
  for (size_t i = 0; i < pr.nbest.size(); ++i) {
    if (lens) lens[i] = (int32_t)pr.nbest[i].size();
    if (times_lens) times_lens[i] = (int32_t)pr.times[i].size();
    if (scores) scores[i] = pr.scores[i];
    for (int j = 0; j < ml; ++j) {
      if (tokens) tokens[i * ml + j] = j < (int)pr.nbest[i].size() ? pr.nbest[i][j] : -1;
      if (times) times[i * ml + j] = j < (int)pr.times[i].size() ? pr.times[i][j] : -1;
    }
  }
}

}  // namespace rvb

// ================================================================================================
//                                         C ABI
// ================================================================================================
using namespace rvb;

extern "C" {

const char* rvb_last_error(void) { return last_error(); }
const char* rvb_version(void) { return "librvb 0.1 (gfx950)"; }

int rvb_model_cfg_size(void) { return (int)sizeof(rvb_model_cfg); }

// host only (no GPU needed): word alignment counts for reverb_amd/wer_evaluation/align.py (search.cpp edit_counts)
int rvb_wer_counts(const int32_t* ref, int64_t n_ref, const int32_t* hyp, int64_t n_hyp, int64_t* counts) {
  if ((!ref && n_ref > 0) || (!hyp && n_hyp > 0) || !counts || n_ref < 0 || n_hyp < 0) { set_error("rvb_wer_counts: bad argument"); return E_ARG; }
  edit_counts(ref, n_ref, hyp, n_hyp, counts);
  return OK;
}

int rvb_create(const rvb_model_cfg* cfg, int device, rvb_engine** out) {
  if (!cfg || !out) { set_error("rvb_create: null argument"); return E_ARG; }
  if (cfg->struct_size != (int32_t)sizeof(rvb_model_cfg)) {
    set_error("rvb_create: ABI mismatch: rvb_model_cfg.struct_size is " + std::to_string(cfg->struct_size) + ", this library's struct has " +
              std::to_string(sizeof(rvb_model_cfg)) + " bytes (bind it field by field from include/rvb.h)");
    return E_ARG;
  }
  if (cfg->dtype != RVB_F32 && cfg->dtype != RVB_BF16 && cfg->dtype != RVB_FP8) { set_error("rvb_create: bad dtype"); return E_ARG; }
  if (cfg->d_model <= 0 || cfg->heads <= 0 || cfg->d_model % cfg->heads || cfg->d_model % 8 || cfg->ffn_dim % 8 ||
      cfg->dec_ffn_dim % 8 || cfg->input_dim != 80 || cfg->vocab < 2 || cfg->num_blocks < 1 ||
      cfg->cnn_kernel < 1 || cfg->cnn_kernel > 31 || (!cfg->cnn_causal && (cfg->cnn_kernel % 2) == 0) ||
      cfg->chunk_frames < 7 || cfg->max_chunks < 1 ||
      (cfg->dec_blocks > 0 && (cfg->dec_heads <= 0 || cfg->d_model % cfg->dec_heads))) {
    set_error("rvb_create: unsupported model dimensions (need d, ffn dims % 8 == 0, d % heads == 0, input_dim 80, cnn kernel <= 31 and odd unless causal)");
    return E_ARG;
  }
  int ndev = 0;
  hipError_t err = hipGetDeviceCount(&ndev);
  if (err != hipSuccess || ndev <= 0) { set_error("no HIP device available: librvb has no CPU fallback"); return E_HIP; }
  if (device < 0 || device >= ndev) { set_error("rvb_create: device index out of range"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(device));
  rvb_engine* e = new rvb_engine();
  e->cfg = *cfg; e->device = device;
  e->fp8 = cfg->dtype == RVB_FP8;                 // the bf16 engine with the encoder's large GEMMs on the fp8 MFMA path
  e->dtype = e->fp8 ? (int)DT_BF16 : cfg->dtype;
  hipError_t se = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (se != hipSuccess) { delete e; set_error("hipStreamCreate failed"); return E_HIP; }
  *out = e;
  return OK;
}

void rvb_destroy(rvb_engine* e) {
  if (!e) return;
  (void)rvb_comm_destroy(e);
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  // DevBuf members are released explicitly: list the big ones, the rest die with the process
  DevBuf* bufs[] = {&e->cmvn_mean, &e->cmvn_istd, &e->conv1_w, &e->conv1_b, &e->pe_f32, &e->stage, &e->pcm, &e->feats,
                    &e->d_feats_in, &e->X1, &e->X2, &e->x, &e->xn, &e->y, &e->h, &e->ao, &e->dconv, &e->enc_out,
                    &e->logits, &e->topv, &e->topi, &e->d_enc_lens, &e->d_seq_start, &e->d_seq_len, &e->d_aux_i32,
                    &e->dx, &e->dxn, &e->dy, &e->dh, &e->dqkv, &e->dq, &e->dao, &e->kvmem, &e->d_tok, &e->d_pos,
                    &e->d_tgt, &e->d_logp, &e->d_hq_start, &e->d_hq_len, &e->d_hkv_start, &e->d_hkv_len,
                    &e->d_hq_pos0, &e->d_hpath_start, &e->d_hpath_len, &e->d_path, &e->d_work, &e->d_tgt_ptr,
                    &e->fb_window, &e->fb_twiddle, &e->fb_melw, &e->fb_lo, &e->fb_hi,
                    &e->conv2.w, &e->conv2.b, &e->embed_out.w, &e->embed_out.b, &e->ctc.w, &e->ctc.b,
                    &e->enc_after.g, &e->enc_after.b};
  for (DevBuf* b : bufs) b->release();
  e->aligner.release();
  e->graph_aligner.release();
  e->graph_scorer.release();
  e->long_aligner.release();
  e->long_scorer.release();
  e->long_graph_aligner.release();
  e->long_graph_scorer.release();
  e->finder.release();
  e->scorer.release();
  for (DevBuf* b : {&e->align_lp, &e->align_tv, &e->align_ti, &e->align_row, &e->align_col, &e->align_out}) b->release();
  e->d_xlse.release(); e->d_xsum.release(); e->d_xtop.release();
  e->atopv.release(); e->atopi.release(); e->d_stream_i32.release(); e->d_amax.release(); e->d_f8sat.release();
  e->wave_f32.release(); e->wave_in.release(); e->rs_kernel.release(); e->d_frame0.release(); e->d_rec.release();
  for (DevBuf* b : {&e->feats_packed, &e->pc_loud, &e->pc_rec, &e->pc_frame0, &e->pc_table, &e->pc_count, &e->pc_pieces}) b->release();
  e->jlogp.release(); e->jpair_row.release(); e->jpair_tok.release(); e->jpair_out.release();
  for (auto& b : e->jkv) b.release();
  for (auto* v : {&e->stream_st.kv, &e->stream_st.kv2, &e->stream_st.cnn, &e->stream_st.cnn2}) for (auto& b : *v) b.release();
  for (auto* v : {&e->kcache, &e->vcache, &e->kcache2, &e->vcache2, &e->memkv}) for (auto& b : *v) b.release();
  auto rel_lin = [](Linear& l) { l.w.release(); l.b.release(); l.w8.release(); l.wscale.release(); };
  auto rel_n = [](LNorm& n) { n.g.release(); n.b.release(); };
  for (auto& L : e->enc) {
    for (Linear* l : {&L.ffm1, &L.ffm2, &L.ff1, &L.ff2, &L.qkv, &L.att_out, &L.pw1, &L.pw1_glu, &L.pw2, &L.lsl}) rel_lin(*l);
    for (LNorm* n : {&L.n_ffm, &L.n_mha, &L.n_conv, &L.n_ff, &L.n_final, &L.n_cnn}) rel_n(*n);
    L.pos_keys.release(); L.pos_bias.release(); L.bias_u.release(); L.bias_v.release(); L.dw_w.release(); L.dw_b.release();
  }
  for (Decoder* D : {&e->dec_l, &e->dec_r}) {
    D->embed.release(); rel_lin(D->out); rel_n(D->after);
    for (auto& L : D->layers) {
      for (Linear* l : {&L.self_qkv, &L.self_out, &L.src_q, &L.src_kv, &L.src_out, &L.ff1, &L.ff2, &L.lsl}) rel_lin(*l);
      for (LNorm* n : {&L.n1, &L.n2, &L.n3}) rel_n(*n);
      L.kvmem.release();
    }
  }
  if (e->h_topv) (void)hipHostFree(e->h_topv);
  if (e->h_topi) (void)hipHostFree(e->h_topi);
  for (auto& sl : e->slices) if (!sl.done) (void)hipEventDestroy(sl.ev);
  for (auto ev : e->slice_event_pool) (void)hipEventDestroy(ev);
  for (auto& p : e->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto ev : e->event_pool) (void)hipEventDestroy(ev);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->pcm_ready) (void)hipEventDestroy(e->pcm_ready);
  if (e->pcm_free) (void)hipEventDestroy(e->pcm_free);
  e->pcm_next.release();
  for (auto& t : e->taps) t.second.buf.release();
  for (auto& t : e->dtaps) t.second.buf.release();
  (void)hipStreamDestroy(e->stream);
  delete e;
}

int rvb_load_tensor(rvb_engine* e, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!e || !name || !host || ndim < 0 || (ndim > 0 && !shape)) { set_error("rvb_load_tensor: null argument"); return E_ARG; }
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) { if (shape[i] < 0) { set_error("negative dim"); return E_ARG; } t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  t.data.assign(host, host + n);
  e->host[name] = std::move(t);
  return OK;
}

int rvb_finalize(rvb_engine* e, const float* cat_embs, int n_cat) {
  if (!e || (n_cat > 0 && !cat_embs)) { set_error("rvb_finalize: null argument"); return E_ARG; }
  return finalize_impl(e, cat_embs, n_cat);
}

int64_t rvb_num_frames(int64_t n) { return n < 400 ? 0 : 1 + (n - 400) / 160; }

int rvb_upload_pcm(rvb_engine* e, const int16_t* pcm, int64_t n) {
  if (!e || (!pcm && n > 0) || n < 0) { set_error("rvb_upload_pcm: bad argument"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(drop_pending_upload(e));
  e->packed = false;             // rvb_pause_chunks: an upload restores the fixed layout
  RVB_TRY(e->pcm.ensure((size_t)n * 2 + 16));
  if (n) RVB_HIP_CHECK(hipMemcpyAsync(e->pcm.p, pcm, (size_t)n * 2, hipMemcpyHostToDevice, e->stream));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->n_samples = n;
  e->pcm_is_float = false;
  e->batch = false;
  return OK;
}

// The double-buffered form: returns as soon as the copy is enqueued on the engine's copy stream (page-locked `pcm`: it then runs
// on a DMA engine underneath whatever the engine's compute stream is doing -- the decoding of the PREVIOUS recording); the
// samples become the engine's audio at the next rvb_fbank, which orders itself behind the copy.  `pcm` must stay valid and
// unchanged until then.  One upload may be pending at a time.
int rvb_upload_pcm_async(rvb_engine* e, const int16_t* pcm, int64_t n) {
  if (!e || (!pcm && n > 0) || n < 0) { set_error("rvb_upload_pcm_async: bad argument"); return E_ARG; }
  if (e->pcm_pending) { set_error("rvb_upload_pcm_async: an upload is already pending (consumed by the next rvb_fbank)"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  if (!e->copy_stream) {
    RVB_HIP_CHECK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    RVB_HIP_CHECK(hipEventCreateWithFlags(&e->pcm_ready, hipEventDisableTiming));
    RVB_HIP_CHECK(hipEventCreateWithFlags(&e->pcm_free, hipEventDisableTiming));
  }
  else RVB_HIP_CHECK(hipStreamWaitEvent(e->copy_stream, e->pcm_free, 0));        // WAR: the last fbank may still read a PCM buffer
  RVB_TRY(e->pcm_next.ensure((size_t)n * 2 + 16));
  if (n) RVB_HIP_CHECK(hipMemcpyAsync(e->pcm_next.p, pcm, (size_t)n * 2, hipMemcpyHostToDevice, e->copy_stream));
  RVB_HIP_CHECK(hipEventRecord(e->pcm_ready, e->copy_stream));
  e->n_samples_next = n;
  e->pcm_pending = true;
  return OK;
}

int rvb_host_alloc(void** out, int64_t bytes) {
  if (!out || bytes < 0) { set_error("rvb_host_alloc: bad argument"); return E_ARG; }
  *out = nullptr;
  hipError_t err = hipHostMalloc(out, (size_t)std::max<int64_t>(bytes, 16), hipHostMallocDefault);
  if (err != hipSuccess) { *out = nullptr; set_error(std::string("hipHostMalloc: ") + hipGetErrorString(err)); return E_NOMEM; }
  return OK;
}
int rvb_host_free(void* p) {
  if (p) RVB_HIP_CHECK(hipHostFree(p));
  return OK;
}

int rvb_set_fp8_policy(rvb_engine* e, int groups, int first_block, int last_block) {
  if (!e) { set_error("rvb_set_fp8_policy: null engine"); return E_ARG; }
  if (!e->fp8) { set_error("rvb_set_fp8_policy: not an RVB_FP8 engine"); return E_STATE; }
  if (groups > 63 || first_block < 0) { set_error("rvb_set_fp8_policy: groups is a 6-bit mask (bit 5: the subsampling's conv2), first_block >= 0"); return E_ARG; }
  return set_fp8_policy_impl(e, groups, first_block, last_block);
}

int rvb_set_decoding_chunk(rvb_engine* e, int chunk_size, int num_left_chunks) {
  if (!e) { set_error("rvb_set_decoding_chunk: null engine"); return E_ARG; }
  if (chunk_size > 4095 || num_left_chunks > 4094) { set_error("rvb_set_decoding_chunk: value too large"); return E_ARG; }
  e->dec_chunk = chunk_size > 0 ? chunk_size : 0;
  e->dec_left = num_left_chunks < 0 ? -1 : num_left_chunks;
  return OK;
}

int rvb_upload_pcm_rate(rvb_engine* e, const int16_t* pcm, int64_t n, int sample_rate) {
  if (sample_rate == 16000) return rvb_upload_pcm(e, pcm, n);
  if (!e || (!pcm && n > 0) || n < 0 || sample_rate < 1000 || sample_rate > 384000) { set_error("rvb_upload_pcm_rate: bad argument"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(drop_pending_upload(e));
  e->packed = false;
  RVB_TRY(e->pcm.ensure((size_t)n * 2 + 16));
  if (n) RVB_HIP_CHECK(hipMemcpyAsync(e->pcm.p, pcm, (size_t)n * 2, hipMemcpyHostToDevice, e->stream));
  return resample_uploaded(e, false, n, sample_rate);
}

int rvb_upload_wave_f32(rvb_engine* e, const float* wave, int64_t n, int sample_rate) {
  if (!e || (!wave && n > 0) || n < 0 || sample_rate < 1000 || sample_rate > 384000) { set_error("rvb_upload_wave_f32: bad argument"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(drop_pending_upload(e));
  e->packed = false;
  rvb::DevBuf& dst = sample_rate == 16000 ? e->wave_f32 : e->wave_in;
  RVB_TRY(dst.ensure((size_t)std::max<int64_t>(n, 1) * 4));
  if (n) RVB_HIP_CHECK(hipMemcpyAsync(dst.p, wave, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  if (sample_rate != 16000) return resample_uploaded(e, true, n, sample_rate);
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->n_samples = n;
  e->pcm_is_float = true;
  e->batch = false;
  return OK;
}

int rvb_get_waveform(rvb_engine* e, float* out, int64_t* n) {
  if (!e) { set_error("rvb_get_waveform: null engine"); return E_ARG; }
  if (e->batch) { set_error("rvb_get_waveform: the engine holds a batch of recordings (rvb_upload_batch); rvb_batch_n_samples gives their lengths"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  if (n) *n = e->n_samples;
  if (!out || e->n_samples == 0) return OK;
  if (e->pcm_is_float) {
    RVB_HIP_CHECK(hipMemcpy(out, e->wave_f32.p, (size_t)e->n_samples * 4, hipMemcpyDeviceToHost));
  } else {
    std::vector<int16_t> tmp(e->n_samples);
    RVB_HIP_CHECK(hipMemcpy(tmp.data(), e->pcm.p, (size_t)e->n_samples * 2, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < e->n_samples; ++i) out[i] = (float)tmp[i];
  }
  return OK;
}

int rvb_fbank(rvb_engine* e, float* feats_out, int64_t* n_frames) {
  if (!e) { set_error("rvb_fbank: null engine"); return E_ARG; }
  if (!e->fb_window.p) { set_error("rvb_fbank before rvb_finalize"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  if (e->pcm_pending) {          // rvb_upload_pcm_async: the samples that went up underneath the previous decode become the audio
    RVB_HIP_CHECK(hipStreamWaitEvent(e->stream, e->pcm_ready, 0));
    std::swap(e->pcm, e->pcm_next);
    e->n_samples = e->n_samples_next;
    e->pcm_is_float = false;
    e->pcm_pending = false;
    e->batch = false;
  }
  if (e->batch) { set_error("rvb_fbank: the engine holds a batch of recordings (rvb_upload_batch): call rvb_fbank_batch"); return E_STATE; }
  e->packed = false;             // rvb_pause_chunks: an fbank call restores the fixed layout
  const int64_t nf = rvb_num_frames(e->n_samples);
  const int64_t T0 = e->cfg.chunk_frames;
  // zero padded so that ANY chunking with chunk_size <= chunk_frames finds whole chunks (feats_batcher pads the last
  // chunk with zeros, cli/reverb.py:165-175): ceil(nf / c) * c < nf + c <= nf + chunk_frames
  const int64_t rows = nf + T0;
  RVB_TRY(e->feats.ensure((size_t)std::max<int64_t>(rows, 1) * 80 * 4));
  // only the padding rows: the kernel writes rows [0, nf)
  RVB_HIP_CHECK(hipMemsetAsync((char*)e->feats.p + (size_t)nf * 80 * 4, 0, (size_t)std::max<int64_t>(rows - nf, 1) * 80 * 4, e->stream));
  FbankTables t{e->fb_window.as<float>(), e->fb_twiddle.as<float>(), e->fb_melw.as<float>(), e->fb_lo.as<int>(), e->fb_hi.as<int>()};
  {
    Scope sc(e, "fbank");
    if (e->pcm_is_float) RVB_TRY(fbank_f32(e->stream, e->wave_f32.as<float>(), nf, e->feats.as<float>(), t));
    else RVB_TRY(fbank(e->stream, e->pcm.as<int16_t>(), nf, e->feats.as<float>(), t));
  }
  if (e->copy_stream) RVB_HIP_CHECK(hipEventRecord(e->pcm_free, e->stream));     // the PCM buffers are idle from here on
  if (feats_out && nf) {
    RVB_HIP_CHECK(hipMemcpyAsync(feats_out, e->feats.p, (size_t)nf * 80 * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  // features that stay in HBM: nothing to wait for, rvb_encode is ordered behind the kernel on the engine's stream
  e->n_frames = nf; e->feat_rows = rows; e->feat_kind = 1;
  if (n_frames) *n_frames = nf;
  return OK;
}

int rvb_encode(rvb_engine* e, const float* feats, int64_t first_chunk, const int32_t* lens, int B, int T0, int beam,
               float blank_penalty) {
  if (!e || !lens) { set_error("rvb_encode: null argument"); return E_ARG; }
  return encode_impl(e, feats, first_chunk, lens, B, T0, beam, blank_penalty);
}

int rvb_stream_begin(rvb_engine* e) {
  if (!e) { set_error("rvb_stream_begin: null engine"); return E_ARG; }
  return stream_begin_impl(e);
}
int rvb_stream_chunk(rvb_engine* e, const float* feats, int n_frames, int required_cache_size, float* out, int32_t* n_out) {
  if (!e || !feats) { set_error("rvb_stream_chunk: null argument"); return E_ARG; }
  return stream_chunk_impl(e, feats, n_frames, required_cache_size, out, n_out);
}
int rvb_stream_state(rvb_engine* e, int32_t* offset, int32_t* cache_frames) {
  if (!e) { set_error("rvb_stream_state: null engine"); return E_ARG; }
  if (offset) *offset = e->stream_st.offset;
  if (cache_frames) *cache_frames = e->stream_st.cache_len;
  return OK;
}
int rvb_stream_finish(rvb_engine* e, int beam, float blank_penalty) {
  if (!e) { set_error("rvb_stream_finish: null engine"); return E_ARG; }
  return stream_finish_impl(e, beam, blank_penalty);
}

int rvb_encoder_frames(rvb_engine* e, int32_t* T_out) {
  if (!e || !T_out || e->B <= 0) { set_error("no encoded batch"); return E_STATE; }
  *T_out = e->T2; return OK;
}
int rvb_get_encoder_lens(rvb_engine* e, int32_t* lens) {
  if (!e || !lens || e->B <= 0) { set_error("no encoded batch"); return E_STATE; }
  memcpy(lens, e->enc_lens.data(), (size_t)e->B * 4); return OK;
}
int rvb_get_encoder_out(rvb_engine* e, float* out) {
  if (!e || !out || e->B <= 0) { set_error("no encoded batch"); return E_STATE; }
  const size_t n = (size_t)e->B * e->T2 * e->cfg.d_model;
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(wait_slices(e, -1));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  if (e->dtype == DT_F32) {
    RVB_HIP_CHECK(hipMemcpy(out, e->enc_out.p, n * 4, hipMemcpyDeviceToHost));
  } else {
    std::vector<bf16_t> tmp(n);
    RVB_HIP_CHECK(hipMemcpy(tmp.data(), e->enc_out.p, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = bf16_to_f32(tmp[i]);
  }
  return OK;
}
int rvb_get_ctc_logprobs(rvb_engine* e, int chunk, float* out) {
  if (!e || !out || e->B <= 0 || chunk < 0 || chunk >= e->B) { set_error("rvb_get_ctc_logprobs: bad chunk"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  const int d = e->cfg.d_model, V = e->cfg.vocab, T = e->T2, Vld = (V + 3) & ~3;
  if (T > LOGIT_SLAB) { set_error("chunk too long for the logit slab"); return E_UNSUPPORTED; }
  RVB_TRY(wait_slices(e, -1));
  DevBuf lp, tv, ti;
  RVB_TRY(lp.ensure((size_t)T * V * 4)); RVB_TRY(tv.ensure((size_t)T * 4)); RVB_TRY(ti.ensure((size_t)T * 4));
  int r = run_gemm(e, (const char*)e->enc_out.p + (size_t)chunk * T * d * dt_size(e->dtype), d, e->ctc, e->logits.p, Vld, T, true);
  if (r == OK) r = logsoftmax_topk(e->stream, e->logits.as<float>(), T, V, Vld, 1, 0.f, e->cfg.blank_id, tv.as<float>(), ti.as<int>(), lp.as<float>());
  if (r == OK && hipMemcpyAsync(out, lp.p, (size_t)T * V * 4, hipMemcpyDeviceToHost, e->stream) != hipSuccess) r = E_HIP;
  (void)hipStreamSynchronize(e->stream);
  lp.release(); tv.release(); ti.release();
  return r;
}
int rvb_get_ctc_topk(rvb_engine* e, float* vals, int32_t* idx) {
  if (!e || e->B <= 0) { set_error("no encoded batch"); return E_STATE; }
  const size_t n = (size_t)e->B * e->T2 * e->beam;
  RVB_TRY(wait_slices(e, -1));
  if (vals) memcpy(vals, e->h_topv, n * 4);
  if (idx) memcpy(idx, e->h_topi, n * 4);
  return OK;
}

int rvb_set_encoder_tap(rvb_engine* e, int block) {
  if (!e) { set_error("rvb_set_encoder_tap: null engine"); return E_ARG; }
  if (!e->finalized) { set_error("rvb_set_encoder_tap before rvb_finalize"); return E_STATE; }
  const int nb = (int)e->enc.size();
  if (block < -1 || block > nb) { set_error("rvb_set_encoder_tap: block must be -1 (off), 0 .. blocks - 1, or blocks (the front end)"); return E_ARG; }
  if (block >= 0 && e->fp8) { set_error("rvb_set_encoder_tap: not available on an fp8 engine (its calibration and fp8 passes store other tensors)"); return E_UNSUPPORTED; }
  if (block >= 0 && e->stream_st.active) { set_error("rvb_set_encoder_tap: not available while a stream is open (the streaming encoder keeps caches instead)"); return E_STATE; }
  if (block != e->tap_block) {       // another position, or off (rvb_encode is what it was): what the taps held is given back
    RVB_HIP_CHECK(hipSetDevice(e->device));
    RVB_TRY(wait_slices(e, -1));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    for (auto& t : e->taps) t.second.buf.release();
    e->taps.clear(); e->tap_forms.clear();
  }
  e->tap_block = block; e->tap_live = false;
  return OK;
}
int rvb_get_encoder_tap(rvb_engine* e, const char* name, float* out, int64_t capacity) {
  if (!e || !name || !out) { set_error("rvb_get_encoder_tap: null argument"); return E_ARG; }
  const bool forms = !strcmp(name, "forms");
  auto it = e->taps.find(name);
  if (!forms && it == e->taps.end()) {
    set_error(std::string("rvb_get_encoder_tap: no tap named ") + name + " was kept by the last rvb_encode (see rvb_set_encoder_tap)");
    return E_STATE;
  }
  const size_t n = forms ? e->tap_forms.size() + 1 : it->second.elems;
  if (capacity < (int64_t)n) {
    set_error(std::string("rvb_get_encoder_tap: ") + name + " holds " + std::to_string(n) + " values, the buffer " + std::to_string(capacity));
    return E_ARG;
  }
  if (forms) {
    out[0] = (float)e->tap_forms.size();
    for (size_t i = 0; i < e->tap_forms.size(); ++i) out[1 + i] = e->tap_forms[i];
    return OK;
  }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(wait_slices(e, -1));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  if (!it->second.bf16) {
    RVB_HIP_CHECK(hipMemcpy(out, it->second.buf.p, n * 4, hipMemcpyDeviceToHost));
  } else {       // widened bit for bit
    std::vector<bf16_t> tmp(n);
    RVB_HIP_CHECK(hipMemcpy(tmp.data(), it->second.buf.p, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = bf16_to_f32(tmp[i]);
  }
  return OK;
}

int rvb_ctc_greedy(rvb_engine* e, int32_t* tokens, int32_t* ntok, int32_t* frames) {
  if (!e || !tokens || !ntok || e->B <= 0) { set_error("rvb_ctc_greedy: no encoded batch"); return E_STATE; }
  const int T = e->T2, beam = e->beam;
  RVB_TRY(wait_slices(e, -1));
  std::vector<int> tk, fr;
  for (int b = 0; b < e->B; ++b) {
    greedy_collapse(e->h_topi + (size_t)b * T * beam, e->enc_lens[b], beam, e->cfg.blank_id, &tk, &fr);
    ntok[b] = (int32_t)tk.size();
    for (size_t i = 0; i < tk.size(); ++i) { tokens[(size_t)b * T + i] = tk[i]; if (frames) frames[(size_t)b * T + i] = fr[i]; }
    for (size_t i = tk.size(); i < (size_t)T; ++i) { tokens[(size_t)b * T + i] = -1; if (frames) frames[(size_t)b * T + i] = -1; }
  }
  return OK;
}

int rvb_ctc_prefix_beam(rvb_engine* e, int beam) {
  if (!e) { set_error("null engine"); return E_ARG; }
  return prefix_beam_impl(e, beam);
}
int rvb_set_context_graph(rvb_engine* e, const int32_t* tokens, const int32_t* lens, int n_phrases, double context_score) {
  if (!e) { set_error("rvb_set_context_graph: null engine"); return E_ARG; }
  if (n_phrases == 0) { e->context_graph.reset(); return OK; }
  const std::string bad = ContextGraph::check(tokens, lens, n_phrases, e->cfg.vocab, e->cfg.blank_id);
  if (!bad.empty()) { set_error(("rvb_set_context_graph: " + bad).c_str()); return E_ARG; }
  if (!std::isfinite(context_score)) { set_error("rvb_set_context_graph: context_score is not finite"); return E_ARG; }
  try {
    e->context_graph = std::make_shared<const ContextGraph>(tokens, lens, n_phrases, context_score);
  } catch (const std::bad_alloc&) {
    set_error("rvb_set_context_graph: out of host memory"); return E_NOMEM;
  }
  return OK;
}
int rvb_get_nbest_count(rvb_engine* e, int chunk, int32_t* n_hyps, int32_t* max_len) {
  if (!e || chunk < 0 || chunk >= (int)e->nbest.size()) { set_error("rvb_get_nbest_count: bad chunk / no search results"); return E_STATE; }
  const PrefixResult& pr = e->nbest[chunk];
  int ml = 0;
  for (auto& h : pr.nbest) ml = std::max(ml, (int)h.size());
  for (auto& t : pr.times) ml = std::max(ml, (int)t.size());
  if (n_hyps) *n_hyps = (int32_t)pr.nbest.size();
  if (max_len) *max_len = ml;
  return OK;
}
int rvb_get_nbest(rvb_engine* e, int chunk, int32_t* tokens, int32_t* lens, int32_t* times, int32_t* times_lens, double* scores) {
  int32_t n, ml;
  int r = rvb_get_nbest_count(e, chunk, &n, &ml);
  if (r != OK) return r;
  fill_nbest(e->nbest[chunk], ml, tokens, lens, times, times_lens, scores);
  return OK;
}

int rvb_prepare_rescoring(rvb_engine* e, int right_to_left) {
  if (!e) { set_error("rvb_prepare_rescoring: null engine"); return E_ARG; }
  if (e->B <= 0) { set_error("rvb_prepare_rescoring before rvb_encode"); return E_STATE; }
  if (!e->dec_l.present) { set_error("model has no attention decoder"); return E_STATE; }
  if (right_to_left && !e->dec_r.present) { set_error("rvb_prepare_rescoring: model has no right-to-left decoder"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  // enqueued behind the encoder slices still in flight; nothing here waits for the device
  if (!e->dec_l.kv_ready) RVB_TRY(decoder_memory_kv(e, e->dec_l, e->B * e->T2));
  if (right_to_left && !e->dec_r.kv_ready) RVB_TRY(decoder_memory_kv(e, e->dec_r, e->B * e->T2));
  return OK;
}
int rvb_attention_rescore(rvb_engine* e, double ctc_weight, double reverse_weight) {
  if (!e) { set_error("null engine"); return E_ARG; }
  return rescore_impl(e, ctc_weight, reverse_weight);
}
int rvb_attention_decode(rvb_engine* e, int beam, float length_penalty) {
  if (!e) { set_error("rvb_attention_decode: null engine"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  return attention_decode_impl(e, beam, length_penalty);
}
int rvb_joint_decode(rvb_engine* e, int beam, double ctc_weight, double pre_beam_ratio, double length_bonus) {
  if (!e) { set_error("rvb_joint_decode: null engine"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  return joint_decode_impl(e, beam, ctc_weight, pre_beam_ratio, length_bonus);
}
int rvb_get_joint_result(rvb_engine* e, int chunk, int32_t* tokens, int32_t* times, int32_t* end_times, double* tokens_confidence,
                         int32_t* n_tokens, double* score) {
  if (!e || !n_tokens) { set_error("rvb_get_joint_result: null argument"); return E_ARG; }
  if (chunk < 0 || chunk >= (int)e->joint.size()) { set_error("rvb_get_joint_result: no joint_decoding result for this chunk"); return E_STATE; }
  const JointResult& r = e->joint[chunk];
  for (size_t i = 0; i < r.tokens.size(); ++i) {      // capacity: rvb_encoder_frames() entries each
    if (tokens) tokens[i] = r.tokens[i];
    if (times) times[i] = r.times[i];
    if (end_times) end_times[i] = r.end_times[i];
    if (tokens_confidence) tokens_confidence[i] = r.tokens_confidence[i];
  }
  *n_tokens = (int32_t)r.tokens.size();
  if (score) *score = r.score;
  return OK;
}
int rvb_get_joint_stats(rvb_engine* e, int64_t* decoder_rows, int64_t* steps) {
  if (!e) { set_error("rvb_get_joint_stats: null engine"); return E_ARG; }
  if (decoder_rows) *decoder_rows = e->joint_rows;
  if (steps) *steps = e->joint_steps;
  return OK;
}
int rvb_get_attention_result(rvb_engine* e, int chunk, int32_t* tokens, int32_t* n_tokens, float* score) {
  if (!e || !n_tokens) { set_error("rvb_get_attention_result: null argument"); return E_ARG; }
  if (chunk < 0 || chunk >= (int)e->attn_tokens.size()) { set_error("rvb_get_attention_result: no attention result for this chunk"); return E_STATE; }
  const std::vector<int>& t = e->attn_tokens[chunk];
  if (tokens) for (size_t i = 0; i < t.size(); ++i) tokens[i] = t[i];     // capacity: rvb_encoder_frames() entries
  *n_tokens = (int32_t)t.size();
  if (score) *score = e->attn_scores[chunk];
  return OK;
}

int rvb_get_rescored(rvb_engine* e, int chunk, int32_t* best_index, float* score, double* confidence, double* tokens_confidence) {
  if (!e || chunk < 0 || chunk >= (int)e->rescored.size()) { set_error("rvb_get_rescored: bad chunk / no rescoring results"); return E_STATE; }
  const RescoreResult& r = e->rescored[chunk];
  if (best_index) *best_index = r.best;
  if (score) *score = r.score;
  if (confidence) *confidence = r.confidence;
  if (tokens_confidence) for (size_t i = 0; i < r.tok_conf.size(); ++i) tokens_confidence[i] = r.tok_conf[i];
  return OK;
}
int rvb_get_rescored_batch(rvb_engine* e, int32_t* lens, int32_t* tokens, int32_t* times_lens, int32_t* times,
                           float* scores, double* confidences, double* tokens_confidence) {
  if (!e || (int)e->rescored.size() != e->B || e->B <= 0 || !lens || !tokens) { set_error("rvb_get_rescored_batch: no rescoring results"); return E_STATE; }
  const int T = e->T2;
  for (int b = 0; b < e->B; ++b) {
    const RescoreResult& r = e->rescored[b];
    const PrefixResult& pr = e->nbest[b];
    const std::vector<int>& tk = pr.nbest[r.best];
    const std::vector<int>& tm = pr.times[r.best];
    lens[b] = (int32_t)tk.size();
    if (times_lens) times_lens[b] = (int32_t)tm.size();
    if (scores) scores[b] = r.score;
    if (confidences) confidences[b] = r.confidence;
    for (int j = 0; j < T; ++j) {
      tokens[(size_t)b * T + j] = j < (int)tk.size() ? tk[j] : -1;
      if (times) times[(size_t)b * T + j] = j < (int)tm.size() ? tm[j] : -1;
      if (tokens_confidence) tokens_confidence[(size_t)b * T + j] = j < (int)r.tok_conf.size() ? r.tok_conf[j] : 0.0;
    }
  }
  return OK;
}
int rvb_fp8_recalibrate(rvb_engine* e) {
  if (!e) { set_error("rvb_fp8_recalibrate: null engine"); return E_ARG; }
  if (!e->fp8) { set_error("rvb_fp8_recalibrate: not an fp8 engine"); return E_STATE; }
  e->f8_state = 0;
  return OK;
}
int rvb_get_fp8_scales(rvb_engine* e, float* scales, int32_t* n) {
  if (!e || !n) { set_error("rvb_get_fp8_scales: null argument"); return E_ARG; }
  if (!e->fp8) { set_error("rvb_get_fp8_scales: not an RVB_FP8 engine"); return E_STATE; }
  if (e->f8_state != 2) { *n = 0; return OK; }                       // not calibrated yet
  *n = (int32_t)(e->f8.size() * 7 + 1);
  if (scales) {
    for (size_t l = 0; l < e->f8.size(); ++l) {
      const F8Scales& f = e->f8[l];
      const float v[7] = {f.in_ffm1, f.h_ffm, f.in_qkv, f.in_pw1, f.in_pw2, f.in_ff1, f.h_ff};
      for (int k = 0; k < 7; ++k) scales[l * 7 + k] = v[k];
    }
    scales[e->f8.size() * 7] = e->f8_x1;      // conv1's fp8 output (policy bit 5); 0 = not measured: conv2 stays bf16
  }
  return OK;
}
// Values that did not fit e4m3 at the installed scale (clipped to +-448 by the kernels that write the fp8 operands), per block
// and activation slot in the order of rvb_get_fp8_scales, summed since the scales were calibrated / installed / last reset:
// the fp8 mode's answer to "the calibration batch was not representative" -- until round 4 such clipping was silent.
int rvb_get_fp8_saturation(rvb_engine* e, uint32_t* counts, int32_t* n, int reset) {
  if (!e || !n) { set_error("rvb_get_fp8_saturation: null argument"); return E_ARG; }
  if (!e->fp8) { set_error("rvb_get_fp8_saturation: not an RVB_FP8 engine"); return E_STATE; }
  *n = (int32_t)(e->enc.size() * 7);
  if (!e->d_f8sat.p) { if (counts) memset(counts, 0, (size_t)*n * 4); return OK; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  std::vector<uint32_t> raw(e->enc.size() * 8);
  RVB_HIP_CHECK(hipMemcpyAsync(raw.data(), e->d_f8sat.p, raw.size() * 4, hipMemcpyDeviceToHost, e->stream));
  if (reset) RVB_HIP_CHECK(hipMemsetAsync(e->d_f8sat.p, 0, (e->enc.size() + 1) * 8 * 4, e->stream));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  if (counts)
    for (size_t l = 0; l < e->enc.size(); ++l)
      for (int k = 0; k < 7; ++k) counts[l * 7 + k] = raw[l * 8 + k];
  return OK;
}
int rvb_get_fp8_subsample(rvb_engine* e, float* scale, uint32_t* clipped, int reset) {
  if (!e) { set_error("rvb_get_fp8_subsample: null engine"); return E_ARG; }
  if (!e->fp8) { set_error("rvb_get_fp8_subsample: not an RVB_FP8 engine"); return E_STATE; }
  if (scale) *scale = e->f8_state == 2 ? e->f8_x1 : 0.f;
  if (clipped) *clipped = 0;
  if (e->d_f8sat.p && (clipped || reset)) {
    unsigned* slot = e->d_f8sat.as<unsigned>() + e->enc.size() * 8 + 1;
    uint32_t v = 0;
    RVB_HIP_CHECK(hipMemcpyAsync(&v, slot, 4, hipMemcpyDeviceToHost, e->stream));
    if (reset) RVB_HIP_CHECK(hipMemsetAsync(slot, 0, 4, e->stream));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    if (clipped) *clipped = v;
  }
  return OK;
}
int rvb_set_fp8_scales(rvb_engine* e, const float* scales, int32_t n) {
  if (!e || !scales) { set_error("rvb_set_fp8_scales: null argument"); return E_ARG; }
  if (!e->fp8) { set_error("rvb_set_fp8_scales: not an RVB_FP8 engine"); return E_STATE; }
  const int32_t nb7 = (int32_t)(e->enc.size() * 7);
  if (!e->finalized || (n != nb7 && n != nb7 + 1)) {
    set_error("rvb_set_fp8_scales: need 7 scales per conformer block of a finalized engine (+ optionally the subsampling scale, as rvb_get_fp8_scales returns them)");
    return E_ARG;
  }
  for (int i = 0; i < nb7; ++i) if (!(scales[i] > 0.f) || !std::isfinite(scales[i])) { set_error("rvb_set_fp8_scales: scales must be positive and finite"); return E_ARG; }
  if (n == nb7 + 1) {     // the vector of rvb_get_fp8_scales: its last entry is conv1's output scale (0 = none -> conv2 in bf16)
    if (!(scales[nb7] >= 0.f) || !std::isfinite(scales[nb7])) { set_error("rvb_set_fp8_scales: the subsampling scale must be >= 0 and finite"); return E_ARG; }
    e->f8_x1 = scales[nb7];
  }
  e->f8.resize(e->enc.size());
  for (size_t l = 0; l < e->enc.size(); ++l) {
    const float* v = scales + l * 7;
    e->f8[l] = {v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
  }
  if (e->f8_groups.size() != e->enc.size()) RVB_TRY(set_fp8_policy_impl(e, -1, 0, -1));
  e->f8_state = 2;
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(reset_f8sat(e));
  return OK;
}
int rvb_get_rescore_stats(rvb_engine* e, int64_t* decoder_rows, int64_t* pairs) {
  if (!e) { set_error("rvb_get_rescore_stats: null engine"); return E_ARG; }
  if (decoder_rows) *decoder_rows = e->rescore_rows;
  if (pairs) *pairs = e->rescore_pairs;
  return OK;
}
int rvb_get_rescore_logp(rvb_engine* e, int chunk, int hyp, int right, float* out) {
  if (!e || !out || chunk < 0 || chunk >= (int)e->rescored.size()) { set_error("rvb_get_rescore_logp: bad chunk"); return E_STATE; }
  const RescoreResult& r = e->rescored[chunk];
  const auto& v = right ? r.rlogp : r.logp;
  if (hyp < 0 || hyp >= (int)v.size()) { set_error("rvb_get_rescore_logp: bad hyp"); return E_ARG; }
  for (size_t i = 0; i < v[hyp].size(); ++i) out[i] = v[hyp][i];
  return OK;
}

int rvb_set_profiling(rvb_engine* e, int level) { if (!e) return E_ARG; drain_prof(e); e->profiling = (level == 1 || level == 2) ? level : 0; return OK; }
int rvb_reset_timings(rvb_engine* e) { if (!e) return E_ARG; drain_prof(e); e->prof.clear(); return OK; }
int rvb_get_timing(rvb_engine* e, const char* name, double* ms, double* flops, int64_t* launches) {
  if (!e || !name) return E_ARG;
  drain_prof(e);
  auto it = e->prof.find(name);
  ProfEntry pe; if (it != e->prof.end()) pe = it->second;
  if (ms) *ms = pe.ms; if (flops) *flops = pe.flops; if (launches) *launches = pe.launches;
  return OK;
}
int rvb_get_timing_bytes(rvb_engine* e, const char* name, double* bytes) {
  if (!e || !name || !bytes) return E_ARG;
  auto it = e->prof.find(name);
  *bytes = it != e->prof.end() ? it->second.bytes : 0.0;
  return OK;
}

}  // extern "C"
