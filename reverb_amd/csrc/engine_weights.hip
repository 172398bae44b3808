// librvb engine, weights: the state dict packed to the compute dtype (and to fp8), the positional and fbank tables, rvb_finalize and
// the fp8 policy.
#include "engine_impl.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace rvb {

// fp32 host matrix -> compute dtype on device
static int pack_T(rvb_engine* e, DevBuf& dst, const float* src, size_t n) {
  RVB_TRY(dst.ensure(n * dt_size(e->dtype)));
  if (e->dtype == DT_F32) {
    RVB_HIP_CHECK(hipMemcpyAsync(dst.p, src, n * 4, hipMemcpyHostToDevice, e->stream));
    return OK;
  }
  RVB_TRY(e->stage.ensure(n * 4));
  RVB_HIP_CHECK(hipMemcpyAsync(e->stage.p, src, n * 4, hipMemcpyHostToDevice, e->stream));
  return convert_f32(e->stream, e->dtype, e->stage.as<float>(), dst.p, n);
}
// f8: also keep an fp8 (OCP e4m3) copy with one scale per output channel: w8[n][k] = rne(w[n][k] / s_n), s_n = max|w[n]| / 448
static int pack_linear(rvb_engine* e, Linear& L, const float* w, const float* b, int out, int in, bool f8 = false) {
  L.out = out; L.in = in;
  RVB_TRY(pack_T(e, L.w, w, (size_t)out * in));
  if (b) RVB_TRY(upload_f32(e, L.b, b, out)); else L.b.release();
  if (f8 && e->fp8 && in % 128 == 0) {
    std::vector<uint8_t> q((size_t)out * in);
    std::vector<float> sc(out);
    for (int n = 0; n < out; ++n) {
      const float* row = w + (size_t)n * in;
      float am = 0.f;
      for (int k = 0; k < in; ++k) am = std::max(am, std::fabs(row[k]));
      const float sn = am > 0.f ? am / 448.f : 1.f;
      sc[n] = sn;
      const float inv = 1.f / sn;
      for (int k = 0; k < in; ++k) q[(size_t)n * in + k] = f32_to_fp8_host(row[k] * inv);
    }
    RVB_TRY(L.w8.ensure(q.size()));
    RVB_HIP_CHECK(hipMemcpyAsync(L.w8.p, q.data(), q.size(), hipMemcpyHostToDevice, e->stream));
    RVB_TRY(upload_f32(e, L.wscale, sc.data(), out));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  return OK;
}

static const HostTensor* find(rvb_engine* e, const std::string& name) {
  auto it = e->host.find(name);
  return it == e->host.end() ? nullptr : &it->second;
}
static int need(rvb_engine* e, const std::string& name, size_t numel, const HostTensor** out) {
  const HostTensor* t = find(e, name);
  if (!t) { set_error("missing tensor: " + name); return E_STATE; }
  if (t->numel() != numel) {
    set_error("tensor " + name + " has " + std::to_string(t->numel()) + " elements, expected " + std::to_string(numel));
    return E_ARG;
  }
  *out = t;
  return OK;
}
static int pack_named_linear(rvb_engine* e, Linear& L, const std::string& p, int out, int in, bool bias = true, bool f8 = false) {
  const HostTensor *w, *b = nullptr;
  RVB_TRY(need(e, p + ".weight", (size_t)out * in, &w));
  if (bias) RVB_TRY(need(e, p + ".bias", out, &b));
  return pack_linear(e, L, w->data.data(), b ? b->data.data() : nullptr, out, in, f8);
}
static int pack_norm(rvb_engine* e, LNorm& n, const std::string& p, int d, float eps) {
  const HostTensor *g, *b;
  RVB_TRY(need(e, p + ".weight", d, &g));
  RVB_TRY(need(e, p + ".bias", d, &b));
  n.eps = eps;
  RVB_TRY(upload_f32(e, n.g, g->data.data(), d));
  return upload_f32(e, n.b, b->data.data(), d);
}
// concatenate several [rows_i, in] linears along the output dim
static int pack_concat(rvb_engine* e, Linear& L, const std::vector<std::string>& names, int out_each, int in, bool f8 = false) {
  std::vector<float> w((size_t)names.size() * out_each * in), b((size_t)names.size() * out_each);
  for (size_t i = 0; i < names.size(); ++i) {
    const HostTensor *tw, *tb;
    RVB_TRY(need(e, names[i] + ".weight", (size_t)out_each * in, &tw));
    RVB_TRY(need(e, names[i] + ".bias", out_each, &tb));
    memcpy(w.data() + i * (size_t)out_each * in, tw->data.data(), (size_t)out_each * in * 4);
    memcpy(b.data() + i * (size_t)out_each, tb->data.data(), (size_t)out_each * 4);
  }
  int r = pack_linear(e, L, w.data(), b.data(), (int)names.size() * out_each, in, f8);
  if (r == OK) (void)hipStreamSynchronize(e->stream);   // w/b go out of scope
  return r;
}
// language-specific layers folded with the category weights: W = sum_i c_i W_i, b = sum_i c_i b_i
// (encoder_layer.py:378-390, decoder_layer.py:319-330 with 1-D cat_embs)
static int pack_lsl(rvb_engine* e, Linear& L, const std::string& p, int d, const float* cat, int ncat) {
  std::vector<float> w((size_t)d * d, 0.f), b(d, 0.f);
  for (int i = 0; i < ncat; ++i) {
    const HostTensor *tw, *tb;
    const std::string n = p + ".language_layers." + std::to_string(i);
    RVB_TRY(need(e, n + ".weight", (size_t)d * d, &tw));
    RVB_TRY(need(e, n + ".bias", d, &tb));
    const float c = cat[i];
    if (i == 0) {
      for (size_t k = 0; k < w.size(); ++k) w[k] = c * tw->data[k];
      for (int k = 0; k < d; ++k) b[k] = c * tb->data[k];
    } else {
      for (size_t k = 0; k < w.size(); ++k) w[k] = w[k] + c * tw->data[k];
      for (int k = 0; k < d; ++k) b[k] = b[k] + c * tb->data[k];
    }
  }
  int r = pack_linear(e, L, w.data(), b.data(), d, d);
  if (r == OK) (void)hipStreamSynchronize(e->stream);
  return r;
}

// sinusoid table, transformer/embedding.py:48-56 (float32 arithmetic as torch does it)
static void make_pe(int rows, int d, std::vector<float>* pe) {
  pe->assign((size_t)rows * d, 0.f);
  const float c = (float)(-(std::log(10000.0) / (double)d));
  for (int i = 0; i < d; i += 2) {
    const float div = std::exp((float)i * c);
    for (int pos = 0; pos < rows; ++pos) {
      const float ang = (float)pos * div;
      (*pe)[(size_t)pos * d + i] = std::sin(ang);
      if (i + 1 < d) (*pe)[(size_t)pos * d + i + 1] = std::cos(ang);
    }
  }
}

// Kaldi mel banks / povey window / FFT twiddles (see oracle/fbank_ref.py for the restatement)
int make_fbank_tables(rvb_engine* e) {
  const int WIN = 400, NFFT = 512, NBIN = 257, NMEL = 80;
  const double PI = 3.14159265358979323846;
  std::vector<float> win(WIN), tw(2 * 256), melw((size_t)NMEL * NBIN, 0.f);
  std::vector<int32_t> lo(NMEL, NBIN), hi(NMEL, 0);
  for (int i = 0; i < WIN; ++i) win[i] = (float)std::pow(0.5 - 0.5 * std::cos(2.0 * PI * i / (WIN - 1)), 0.85);
  for (int k = 0; k < 256; ++k) { tw[2 * k] = (float)std::cos(2.0 * PI * k / NFFT); tw[2 * k + 1] = (float)(-std::sin(2.0 * PI * k / NFFT)); }
  auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
  const double mlo = mel(20.0), mhi = mel(8000.0), delta = (mhi - mlo) / (NMEL + 1);
  for (int m = 0; m < NMEL; ++m) {
    const double left = mlo + m * delta, center = left + delta, right = center + delta;
    for (int b = 0; b < NFFT / 2; ++b) {
      const double mf = mel(16000.0 / NFFT * b);
      const double up = (mf - left) / (center - left), down = (right - mf) / (right - center);
      const double w = std::max(0.0, std::min(up, down));
      if (w > 0.0) {
        melw[(size_t)m * NBIN + b] = (float)w;
        lo[m] = std::min(lo[m], b); hi[m] = std::max(hi[m], b + 1);
      }
    }
    if (hi[m] == 0) lo[m] = 0;
  }
  RVB_TRY(upload_f32(e, e->fb_window, win.data(), win.size()));
  RVB_TRY(upload_f32(e, e->fb_twiddle, tw.data(), tw.size()));
  RVB_TRY(upload_f32(e, e->fb_melw, melw.data(), melw.size()));
  RVB_TRY(upload_i32(e, e->fb_lo, lo.data(), lo.size()));
  RVB_TRY(upload_i32(e, e->fb_hi, hi.data(), hi.size()));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  return OK;
}

static int out_frames(int T0) { const int T1 = (T0 - 3) / 2 + 1; return (T1 - 3) / 2 + 1; }

// ------------------------------------------------------------------------------------ finalize
static int pack_decoder(rvb_engine* e, Decoder& D, const std::string& p, int nblocks, const float* cat, int ncat) {
  const int d = e->cfg.d_model, V = e->cfg.vocab, ff = e->cfg.dec_ffn_dim;
  D.present = false;
  if (nblocks <= 0 || !find(e, p + ".embed.0.weight")) return OK;
  const HostTensor* emb;
  RVB_TRY(need(e, p + ".embed.0.weight", (size_t)V * d, &emb));
  RVB_TRY(upload_f32(e, D.embed, emb->data.data(), emb->data.size()));
  RVB_TRY(pack_norm(e, D.after, p + ".after_norm", d, 1e-5f));
  RVB_TRY(pack_named_linear(e, D.out, p + ".output_layer", V, d));
  D.layers.resize(nblocks);
  for (int j = 0; j < nblocks; ++j) {
    DecLayer& L = D.layers[j];
    const std::string q = p + ".decoders." + std::to_string(j);
    L.is_lsl = find(e, q + ".language_layers.0.weight") != nullptr;
    const float eps = L.is_lsl ? 1e-12f : 1e-5f;   // decoder_layer.py:56-58 vs :241-243
    RVB_TRY(pack_concat(e, L.self_qkv, {q + ".self_attn.linear_q", q + ".self_attn.linear_k", q + ".self_attn.linear_v"}, d, d));
    RVB_TRY(pack_named_linear(e, L.self_out, q + ".self_attn.linear_out", d, d));
    RVB_TRY(pack_named_linear(e, L.src_q, q + ".src_attn.linear_q", d, d));
    RVB_TRY(pack_concat(e, L.src_kv, {q + ".src_attn.linear_k", q + ".src_attn.linear_v"}, d, d));
    RVB_TRY(pack_named_linear(e, L.src_out, q + ".src_attn.linear_out", d, d));
    RVB_TRY(pack_named_linear(e, L.ff1, q + ".feed_forward.w_1", ff, d));
    RVB_TRY(pack_named_linear(e, L.ff2, q + ".feed_forward.w_2", d, ff));
    RVB_TRY(pack_norm(e, L.n1, q + ".norm1", d, eps));
    RVB_TRY(pack_norm(e, L.n2, q + ".norm2", d, eps));
    RVB_TRY(pack_norm(e, L.n3, q + ".norm3", d, eps));
    if (L.is_lsl) RVB_TRY(pack_lsl(e, L.lsl, q, d, cat, ncat));
  }
  D.present = true;
  return OK;
}

int finalize_impl(rvb_engine* e, const float* cat, int ncat) {
  const rvb_model_cfg& c = e->cfg;
  const int d = c.d_model, ff = c.ffn_dim, K = c.cnn_kernel, V = c.vocab, F0 = c.input_dim;
  const int F1 = (F0 - 3) / 2 + 1, F2 = (F1 - 3) / 2 + 1;
  if (c.num_langs > 0 && ncat != c.num_langs) { set_error("finalize: cat_embs length must equal num_langs"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));

  if (!e->finalized) {
    const HostTensor *t, *t2;
    RVB_TRY(need(e, "encoder.global_cmvn.mean", F0, &t));
    RVB_TRY(upload_f32(e, e->cmvn_mean, t->data.data(), F0));
    RVB_TRY(need(e, "encoder.global_cmvn.istd", F0, &t));
    RVB_TRY(upload_f32(e, e->cmvn_istd, t->data.data(), F0));
    RVB_TRY(need(e, "encoder.embed.conv.0.weight", (size_t)d * 9, &t));
    {   // tap-major [9][d]: a thread of conv1_kernel reads its 8 channels of a tap as 32 contiguous bytes
      std::vector<float> wt((size_t)d * 9);
      for (int c = 0; c < d; ++c)
        for (int k = 0; k < 9; ++k) wt[(size_t)k * d + c] = t->data[(size_t)c * 9 + k];
      RVB_TRY(upload_f32(e, e->conv1_w, wt.data(), (size_t)d * 9));
    }
    RVB_TRY(need(e, "encoder.embed.conv.0.bias", d, &t));
    RVB_TRY(upload_f32(e, e->conv1_b, t->data.data(), d));
    {  // conv2 [co][ci][kh][kw] -> [co][(kh*3+kw)*d + ci]  (K-contiguous rows for the implicit GEMM)
      RVB_TRY(need(e, "encoder.embed.conv.2.weight", (size_t)d * d * 9, &t));
      RVB_TRY(need(e, "encoder.embed.conv.2.bias", d, &t2));
      std::vector<float> w((size_t)d * 9 * d);
      for (int co = 0; co < d; ++co)
        for (int ci = 0; ci < d; ++ci)
          for (int k = 0; k < 9; ++k) w[((size_t)co * 9 + k) * d + ci] = t->data[((size_t)co * d + ci) * 9 + k];
      RVB_TRY(pack_linear(e, e->conv2, w.data(), t2->data.data(), d, 9 * d, true));      // + fp8 copy in RVB_FP8 mode (policy bit 5)
      RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    {  // out.0 [o][c*F2+f] -> [o][f*d+c]: our conv2 output is (t, f, c) not the reference's (t, c, f)
      RVB_TRY(need(e, "encoder.embed.out.0.weight", (size_t)d * d * F2, &t));
      RVB_TRY(need(e, "encoder.embed.out.0.bias", d, &t2));
      std::vector<float> w((size_t)d * d * F2);
      for (int o = 0; o < d; ++o)
        for (int cc = 0; cc < d; ++cc)
          for (int f = 0; f < F2; ++f) w[(size_t)o * d * F2 + (size_t)f * d + cc] = t->data[(size_t)o * d * F2 + (size_t)cc * F2 + f];
      RVB_TRY(pack_linear(e, e->embed_out, w.data(), t2->data.data(), d, d * F2));
      RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    RVB_TRY(pack_norm(e, e->enc_after, "encoder.after_norm", d, 1e-5f));
    RVB_TRY(pack_named_linear(e, e->ctc, "ctc.ctc_lo", V, d));

    // sinusoid table for encoder positions and decoder positions
    const int Tmax = out_frames(c.chunk_frames);
    // 5000 rows = the reference's positional table (`max_len`, embedding.py:33,130): streaming offsets index it absolutely
    e->pe_rows = std::max(Tmax + 2, 5000);
    std::vector<float> pe;
    make_pe(e->pe_rows, d, &pe);
    RVB_TRY(upload_f32(e, e->pe_f32, pe.data(), pe.size()));
    DevBuf pe_T;
    RVB_TRY(pack_T(e, pe_T, pe.data(), pe.size()));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));

    e->enc.resize(c.num_blocks);
    for (int i = 0; i < c.num_blocks; ++i) {
      EncLayer& L = e->enc[i];
      const std::string p = "encoder.encoders." + std::to_string(i);
      L.is_lsl = find(e, p + ".language_layers.0.weight") != nullptr;
      // fp8 mode: the GEMMs whose A operand is written by a LayerNorm or by a GEMM epilogue (95 % of a block's GEMM work);
      // the language-specific blocks keep their second feed-forward in bf16 (its input is the mixed projection y)
      RVB_TRY(pack_named_linear(e, L.ffm1, p + ".feed_forward_macaron.w_1", ff, d, true, true));
      RVB_TRY(pack_named_linear(e, L.ffm2, p + ".feed_forward_macaron.w_2", d, ff, true, true));
      RVB_TRY(pack_named_linear(e, L.ff1, p + ".feed_forward.w_1", ff, d, true, !L.is_lsl));
      RVB_TRY(pack_named_linear(e, L.ff2, p + ".feed_forward.w_2", d, ff, true, !L.is_lsl));
      RVB_TRY(pack_concat(e, L.qkv, {p + ".self_attn.linear_q", p + ".self_attn.linear_k", p + ".self_attn.linear_v"}, d, d, true));
      RVB_TRY(pack_named_linear(e, L.att_out, p + ".self_attn.linear_out", d, d));
      RVB_TRY(pack_named_linear(e, L.pw1, p + ".conv_module.pointwise_conv1", 2 * d, d, true, true));
      if (e->dtype == DT_BF16) {      // the same weights with rows (c, c + d) next to each other: columns 2c / 2c + 1 of the ACT_GLU GEMM
        const HostTensor *tw, *tb;
        RVB_TRY(need(e, p + ".conv_module.pointwise_conv1.weight", (size_t)2 * d * d, &tw));
        RVB_TRY(need(e, p + ".conv_module.pointwise_conv1.bias", (size_t)2 * d, &tb));
        std::vector<float> wi((size_t)2 * d * d), bi((size_t)2 * d);
        for (int c = 0; c < d; ++c) {
          memcpy(&wi[(size_t)(2 * c) * d], &tw->data[(size_t)c * d], (size_t)d * 4);
          memcpy(&wi[(size_t)(2 * c + 1) * d], &tw->data[(size_t)(d + c) * d], (size_t)d * 4);
          bi[2 * c] = tb->data[c]; bi[2 * c + 1] = tb->data[d + c];
        }
        RVB_TRY(pack_linear(e, L.pw1_glu, wi.data(), bi.data(), 2 * d, d, false));
        RVB_HIP_CHECK(hipStreamSynchronize(e->stream));      // wi / bi go out of scope
      }
      RVB_TRY(pack_named_linear(e, L.pw2, p + ".conv_module.pointwise_conv2", d, d, true, true));
      RVB_TRY(need(e, p + ".self_attn.pos_bias_u", d, &t));
      RVB_TRY(upload_f32(e, L.bias_u, t->data.data(), d));
      RVB_TRY(need(e, p + ".self_attn.pos_bias_v", d, &t));
      RVB_TRY(upload_f32(e, L.bias_v, t->data.data(), d));
      RVB_TRY(need(e, p + ".conv_module.depthwise_conv.weight", (size_t)d * K, &t));
      {   // tap-major [K][d] on the device: the lanes of glu_dw_kernel own adjacent channels, so a tap is one coalesced load
        std::vector<float> wt((size_t)d * K);
        for (int c = 0; c < d; ++c)
          for (int k = 0; k < K; ++k) wt[(size_t)k * d + c] = t->data[(size_t)c * K + k];
        RVB_TRY(upload_f32(e, L.dw_w, wt.data(), (size_t)d * K));
      }
      RVB_TRY(need(e, p + ".conv_module.depthwise_conv.bias", d, &t));
      RVB_TRY(upload_f32(e, L.dw_b, t->data.data(), d));
      RVB_TRY(pack_norm(e, L.n_ffm, p + ".norm_ff_macaron", d, 1e-5f));
      RVB_TRY(pack_norm(e, L.n_mha, p + ".norm_mha", d, 1e-5f));
      RVB_TRY(pack_norm(e, L.n_conv, p + ".norm_conv", d, 1e-5f));
      RVB_TRY(pack_norm(e, L.n_ff, p + ".norm_ff", d, 1e-5f));
      RVB_TRY(pack_norm(e, L.n_final, p + ".norm_final", d, 1e-5f));
      if (c.cnn_norm == 0) {
        RVB_TRY(pack_norm(e, L.n_cnn, p + ".conv_module.norm", d, 1e-5f));
      } else {  // BatchNorm1d (eval) folded to y = x*g' + b'
        const HostTensor *g, *b, *rm, *rv;
        RVB_TRY(need(e, p + ".conv_module.norm.weight", d, &g));
        RVB_TRY(need(e, p + ".conv_module.norm.bias", d, &b));
        RVB_TRY(need(e, p + ".conv_module.norm.running_mean", d, &rm));
        RVB_TRY(need(e, p + ".conv_module.norm.running_var", d, &rv));
        std::vector<float> gg(d), bb(d);
        for (int k = 0; k < d; ++k) {
          gg[k] = g->data[k] / std::sqrt(rv->data[k] + 1e-5f);
          bb[k] = b->data[k] - rm->data[k] * gg[k];
        }
        RVB_TRY(upload_f32(e, L.n_cnn.g, gg.data(), d));
        RVB_TRY(upload_f32(e, L.n_cnn.b, bb.data(), d));
        RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
      }
      // positional keys P = linear_pos(pe[:Tmax]) -- input independent (attention.py:374, embedding.py:145)
      Linear lp;
      RVB_TRY(pack_named_linear(e, lp, p + ".self_attn.linear_pos", d, d, false));
      RVB_TRY(L.pos_keys.ensure((size_t)e->pe_rows * d * dt_size(e->dtype)));
      RVB_TRY(run_gemm(e, pe_T.p, d, lp, L.pos_keys.p, d, e->pe_rows, false));
      if (e->dtype == DT_BF16) {
        // the positional product folded into a per-key constant (attention.hip FOLD): (v - u) . p_j, in the exp2 domain of the kernel
        const int dk_enc = d / c.heads;
        RVB_TRY(L.pos_bias.ensure((size_t)c.heads * e->pe_rows * 4));
        RVB_TRY(attention_pos_bias(e->stream, L.pos_keys.p, e->pe_rows, d, L.bias_u.as<float>(), L.bias_v.as<float>(), c.heads, dk_enc,
                                   1.44269504f / std::sqrt((float)dk_enc), L.pos_bias.as<float>()));
      }
      RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
      lp.w.release(); lp.b.release();
    }
    pe_T.release();
    RVB_TRY(make_fbank_tables(e));
  }
  // (re)fold the language-specific layers with the requested category weights
  for (int i = 0; i < c.num_blocks; ++i) {
    EncLayer& L = e->enc[i];
    if (L.is_lsl) RVB_TRY(pack_lsl(e, L.lsl, "encoder.encoders." + std::to_string(i), d, cat, ncat));
  }
  if (!e->finalized) {
    RVB_TRY(pack_decoder(e, e->dec_l, "decoder.left_decoder", c.dec_blocks, cat, ncat));
    RVB_TRY(pack_decoder(e, e->dec_r, "decoder.right_decoder", c.dec_r_blocks, cat, ncat));
  } else {
    for (int side = 0; side < 2; ++side) {
      Decoder& D = side ? e->dec_r : e->dec_l;
      const std::string p = side ? "decoder.right_decoder" : "decoder.left_decoder";
      if (!D.present) continue;
      for (size_t j = 0; j < D.layers.size(); ++j)
        if (D.layers[j].is_lsl) RVB_TRY(pack_lsl(e, D.layers[j].lsl, p + ".decoders." + std::to_string(j), d, cat, ncat));
    }
  }
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  if (e->fp8) {
    for (auto& L : e->enc)
      if (!L.ffm1.w8.p || !L.ffm2.w8.p || !L.qkv.w8.p || !L.pw1.w8.p || !L.pw2.w8.p || (!L.is_lsl && (!L.ff1.w8.p || !L.ff2.w8.p))) {
        set_error("fp8 mode needs encoder_conf.output_size and linear_units to be multiples of 128 (one fp8 K step)");
        return E_UNSUPPORTED;
      }
  }
  if (!e->finalized) {   // keep only what a later re-finalize needs
    for (auto it = e->host.begin(); it != e->host.end();) {
      if (it->first.find(".language_layers.") == std::string::npos) it = e->host.erase(it); else ++it;
    }
  }
  e->prof.clear();
  e->finalized = true;
  return OK;
}

// Which GEMM groups of which conformer blocks run in fp8 (rvb_set_fp8_policy).  Default: the two feed-forward modules
// (groups 1 | 16) of every block.  Measured on the bench hour against the unmodified reference (profiles/r03_fp8_policy_sweep.txt):
// all five groups 16.2 % greedy / 13.5 % rescored token errors at 123.4 ms; feed-forward only 9.3 % / 10.9 % at 130.8 ms
// (bf16: 4.7 % / 8.9 % at 143.3 ms; the reference's own bf16 autocast: 8.9 % / 9.1 %); qkv + pointwise only 16.4 % / 14.0 %:
// the operands of the softmax (qkv) and of the GLU gate / depthwise path (pointwise 1, 2) are where a 3-bit mantissa hurts.
int set_fp8_policy_impl(rvb_engine* e, int groups, int first_block, int last_block) {
  const int nb = (int)e->enc.size();
  if (nb == 0) { set_error("rvb_set_fp8_policy before rvb_finalize"); return E_STATE; }
  unsigned mask = groups < 0 ? (lab_env("RVB_FP8_GROUPS") ? (unsigned)atoi(lab_env("RVB_FP8_GROUPS")) : 17u) : (unsigned)groups;
  if (groups < 0) {
    if (lab_env("RVB_FP8_FIRST")) first_block = atoi(lab_env("RVB_FP8_FIRST"));
    if (lab_env("RVB_FP8_LAST")) last_block = atoi(lab_env("RVB_FP8_LAST"));
  }
  if (last_block < 0) last_block = nb - 1;
  e->f8_groups.assign(nb, 0u);
  for (int l = 0; l < nb; ++l)
    if (l >= first_block && l <= last_block) e->f8_groups[l] = mask & 31u;
  e->f8_conv2 = (mask & 32u) != 0;           // not per block: the subsampling's conv2
  return OK;
}

}  // namespace rvb
