// librvb engine, encoder: one conformer block, the offline batch encoder with its CTC head (rvb_encode) and the streaming encoder.
#include "engine_impl.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace rvb {

static constexpr int DW_FUSE_DEFAULT = 1;       // depthwise conv + LayerNorm + SiLU in one kernel (encoder_layer: lab switch RVB_DW_FUSE)
static constexpr int GLU_FUSE_DEFAULT = 1;     // pointwise_conv1 + GLU in the GEMM's epilogue (encoder_layer: lab switch RVB_GLU_FUSE)

// ------------------------------------------------------------------------------------ encoder
// One conformer block.  On entry e->xn already holds norm_ff_macaron(x) (written by the previous block's fused final
// norm, or by encode_impl for the first block); on exit the block has written `next`(x) to next_out the same way.
// `li` >= 0 selects the streaming form (forward_chunk, encoder.py:231-341): this chunk's keys / values are appended to
// layer li's cache and attention runs over cache + chunk, positional keys taken at the frames' absolute positions.
// fp8 mode (e->f8_state 2, offline only): the LayerNorms write fp8 operands at the calibrated per-tensor scales, the
// feed-forward / qkv / pointwise GEMMs run on the fp8 MFMA path, intermediate h stays fp8; state 1 is the calibration
// pass: the bf16 flow with the running max |.| of every tensor that will be quantised.
static int encoder_layer(rvb_engine* e, EncLayer& L, int lidx, int M, int B, int T, const LNorm& next, void* next_out,
                         float next8 = 0.f, int li = -1) {
  const int d = e->cfg.d_model, ff = e->cfg.ffn_dim, heads = e->cfg.heads, dk = d / heads;
  float* x = e->x.as<float>();
  const bool f8 = e->fp8 && e->f8_state == 2 && li < 0;
  const bool cal = e->fp8 && e->f8_state == 1 && li < 0;
  // read-only taps of this block (rvb_set_encoder_tap; off: tap_keep / tap_note_gemm return at once): every stored tensor is copied
  // out on the engine's stream behind the launch that wrote it, before the next block overwrites it
  struct TapLive { rvb_engine* e; ~TapLive() { e->tap_live = false; } } tap_guard{e};
  e->tap_live = e->tap_block == lidx && li < 0;
  const bool t16 = e->dtype == DT_BF16;
  const size_t Md = (size_t)M * d;
  RVB_TRY(tap_keep(e, "x_in", x, Md, false));
  RVB_TRY(tap_keep(e, "xn_ffm", e->xn.p, Md, t16));
  // which GEMM groups of this block run in fp8 (rvb_engine::f8_groups: bit 0 macaron feed-forward, 1 qkv, 2 pointwise conv 1,
  // 3 pointwise conv 2, 4 feed-forward); the others stay on the bf16 path, LayerNorm output included
  const unsigned grp = f8 ? e->f8_groups[lidx] : 0u;
  const bool f8_ffm = grp & 1u, f8_qkv = grp & 2u, f8_pw1 = grp & 4u, f8_pw2 = grp & 8u, f8_ff = (grp & 16u) && !L.is_lsl;
  const F8Scales sc8 = f8 ? e->f8[lidx] : F8Scales();
  // Folded rel-pos attention with the fold done by the qkv GEMM (round 6): (q+u).k + (q+v).p = (q+u).(k+p) + (v-u).p; the GEMM's
  // epilogue writes K' = k + p (positional key of the frame's place in its chunk, GemmArgs::rowadd) and the attention kernel
  // (attention.hip FOLD 2) multiplies once per key tile and starts from the per-key constants (v-u).p built at load time.
  // bf16 offline batches only (the streaming form caches k itself, and its positional rows move with the stream offset).
  const char* prefold_env = lab_env("RVB_ATTN_PREFOLD");       // read per call (not cached): the A/B test flips it inside one process
  const int prefold_on = prefold_env ? atoi(prefold_env) : 1;
  const bool prefold = prefold_on && e->dtype == DT_BF16 && li < 0 && !f8_qkv && L.pos_bias.p != nullptr && dk > 32 && dk <= 64 &&
                       T <= e->pe_rows && T <= 16384 && (d % 8) == 0;     // 16384: the keys whose constants the kernel holds in LDS
  if (e->tap_live) {
    e->tap_forms.assign(2, 0.f);
    e->tap_forms[0] = prefold ? 1.f : 0.f;
    RVB_TRY(tap_keep(e, "pos_keys", L.pos_keys.p, (size_t)T * d, t16));
    if (L.pos_bias.p) {       // [heads][pe_rows] -> [heads][T]
      auto& t = e->taps["pos_bias"];
      RVB_TRY(t.buf.ensure((size_t)heads * T * 4));
      t.elems = (size_t)heads * T; t.bf16 = false;
      RVB_HIP_CHECK(hipMemcpy2DAsync(t.buf.p, (size_t)T * 4, L.pos_bias.p, (size_t)e->pe_rows * 4, (size_t)T * 4, heads, hipMemcpyDeviceToDevice, e->stream));
    }
  }
  auto note = [&](int slot, const void* t, size_t n) -> int {
    return cal ? amax_abs(e->stream, e->dtype, t, n, e->d_amax.as<float>() + (size_t)lidx * 8 + slot) : OK;
  };
  // saturation counter of activation slot `slot` of this block (same slot numbering as the scales: in_ffm1, h_ffm, in_qkv,
  // in_pw1, in_pw2, in_ff1, h_ff): the kernels that write an fp8 tensor add the values they had to clip at +-448
  auto satp = [&](int slot) -> unsigned* { return e->d_f8sat.p ? e->d_f8sat.as<unsigned>() + (size_t)lidx * 8 + slot : nullptr; };
  // macaron feed-forward: x += 0.5 * FFN(LN(x))          encoder_layer.py:199-206
  if (f8_ffm) {
    RVB_TRY(run_gemm8(e, e->xn.p, d, L.ffm1, e->h.p, ff, M, sc8.in_ffm1, 2, sc8.h_ffm, 1.f, ACT_SILU, nullptr, 0, satp(1)));
    RVB_TRY(run_gemm8(e, e->h.p, ff, L.ffm2, x, d, M, sc8.h_ffm, 1, 1.f, 0.5f, ACT_NONE, x, d));
  } else {
    RVB_TRY(note(0, e->xn.p, (size_t)M * d));
    RVB_TRY(run_gemm(e, e->xn.p, d, L.ffm1, e->h.p, ff, M, false, 1.f, ACT_SILU));
    RVB_TRY(note(1, e->h.p, (size_t)M * ff));
    RVB_TRY(tap_keep(e, "h_ffm", e->h.p, (size_t)M * ff, t16));
    RVB_TRY(run_gemm(e, e->h.p, ff, L.ffm2, x, d, M, true, 0.5f, ACT_NONE, x, d));
  }
  RVB_TRY(tap_keep(e, "x_ffm", x, Md, false));
  // rel-pos self attention: x += MHSA(LN(x))              encoder_layer.py:208-216
  if (f8_qkv) {
    RVB_TRY(run_norm(e, x, L.n_mha, e->xn.p, false, M, d, NORM_LN, 0, nullptr, nullptr, nullptr, sc8.in_qkv, 0.f, false, satp(2)));
    RVB_TRY(run_gemm8(e, e->xn.p, d, L.qkv, e->h.p, 3 * d, M, sc8.in_qkv, 0));
  } else {
    RVB_TRY(run_norm(e, x, L.n_mha, e->xn.p, false, M, d));
    RVB_TRY(note(2, e->xn.p, (size_t)M * d));
    if (prefold) {       // the K third of the output is written as K' = k + p (one rounding), see `prefold` above
      GemmArgs g;
      memset(&g, 0, sizeof(g));
      g.A = e->xn.p; g.W = L.qkv.w.p; g.bias = L.qkv.b.as<float>(); g.C = e->h.p;
      g.M = M; g.N = 3 * d; g.K = d; g.lda = d; g.ldw = d; g.ldc = 3 * d; g.alpha = 1.f; g.act = ACT_NONE;
      g.rowadd = L.pos_keys.p; g.rowadd_rows = T; g.rowadd_ld = d; g.rowadd_col0 = d; g.rowadd_cols = d;
      Scope sc(e, "gemm", 2.0 * M * (double)g.N * g.K, gemm_alg_bytes(e, g));
      RVB_TRY(gemm(e->stream, e->dtype, g));
      tap_note_gemm(e);
    } else {
      RVB_TRY(run_gemm(e, e->xn.p, d, L.qkv, e->h.p, 3 * d, M, false));
    }
  }
  RVB_TRY(tap_keep(e, "xn_mha", e->xn.p, Md, t16));
  RVB_TRY(tap_keep(e, "qkv", e->h.p, 3 * Md, t16));
  {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    const size_t es = dt_size(e->dtype);
    a.q = e->h.p; a.k = (const char*)e->h.p + (size_t)d * es; a.v = (const char*)e->h.p + (size_t)2 * d * es;
    a.p = L.pos_keys.p;
    {   // bf16: positional term folded into per-key constants (RVB_ATTN_FOLD=1; default: the two-product form)
      static const int fold = lab_env("RVB_ATTN_FOLD") ? atoi(lab_env("RVB_ATTN_FOLD")) : 0;     // measured slower (10.3 -> 10.8 ms per hour): opt-in
      const int cap = (T + 63) / 64 * 64;             // offline: every chunk's keys are its own T frames
      if (fold && li < 0 && L.pos_bias.p && cap <= 16384) { a.pos_bias = L.pos_bias.as<float>(); a.pos_bias_stride = e->pe_rows; a.fold_kv_cap = cap; }
      if (prefold && cap <= 16384) { a.pos_bias = L.pos_bias.as<float>(); a.pos_bias_stride = e->pe_rows; a.k_prefolded = 1; a.fold_kv_cap = cap; }
    }
    a.q_stride = a.k_stride = a.v_stride = 3 * d; a.p_stride = d; a.o_stride = d;
    a.bias_u = L.bias_u.as<float>(); a.bias_v = L.bias_v.as<float>();
    a.out = e->ao.p;
    a.q_start = e->d_seq_start.as<int>(); a.q_len = e->d_seq_len.as<int>();
    a.kv_start = e->d_seq_start.as<int>(); a.kv_len = e->cur_lens;
    a.nseq = B; a.heads = heads; a.dk = dk; a.max_q = T; a.causal = 0; a.sqrt_dk = std::sqrt((float)dk);
    a.chunk = e->dec_chunk; a.left = e->dec_left;          // add_optional_chunk_mask, encoder.py:140-145
    { static const int qb = lab_env("RVB_ATTN_QBLOCK") ? atoi(lab_env("RVB_ATTN_QBLOCK")) : 0; a.q_block = qb; }   // tuning: 64 / 128 queries per workgroup
    double keys = T;
    if (li >= 0) {
      // attention.py:361-369: k = cat(key_cache, k), v = cat(value_cache, v); pos_emb = position_encoding(offset -
      // cache_t1, cache_t1 + chunk) (encoder.py:305-306), no mask (att_mask is the fake (0,0,0) one)
      auto& st = e->stream_st;
      char* kvb = (char*)st.kv[li].p;
      RVB_HIP_CHECK(hipMemcpy2DAsync(kvb + (size_t)st.cache_len * 2 * d * es, (size_t)2 * d * es, (const char*)e->h.p + (size_t)d * es,
                                     (size_t)3 * d * es, (size_t)2 * d * es, M, hipMemcpyDeviceToDevice, e->stream));
      a.k = kvb; a.v = kvb + (size_t)d * es; a.k_stride = a.v_stride = 2 * d;
      a.p = (const char*)L.pos_keys.p + (size_t)(st.offset - st.cache_len) * d * es;
      if (a.pos_bias) a.pos_bias += (st.offset - st.cache_len);
      a.kv_start = e->d_stream_i32.as<int>(); a.kv_len = e->d_stream_i32.as<int>() + 1;
      a.chunk = 0; a.left = -1;
      keys = st.cache_len + M;
    }
    Scope sc(e, "attention", 6.0 * B * (double)T * keys * d);
    RVB_TRY(attention(e->stream, e->dtype, with_lab(a)));
  }
  RVB_TRY(tap_keep(e, "ao", e->ao.p, Md, t16));
  RVB_TRY(run_gemm(e, e->ao.p, d, L.att_out, x, d, M, true, 1.f, ACT_NONE, x, d));
  RVB_TRY(tap_keep(e, "x_att", x, Md, false));
  // convolution module: x += Conv(LN(x))                   encoder_layer.py:218-229, convolution.py:89-144
  bool glu_fused = false;
  if (f8_pw1) {
    RVB_TRY(run_norm(e, x, L.n_conv, e->xn.p, false, M, d, NORM_LN, 0, nullptr, nullptr, nullptr, sc8.in_pw1, 0.f, false, satp(3)));
    RVB_TRY(run_gemm8(e, e->xn.p, d, L.pw1, e->h.p, 2 * d, M, sc8.in_pw1, 0));
  } else {
    RVB_TRY(run_norm(e, x, L.n_conv, e->xn.p, false, M, d));
    RVB_TRY(note(3, e->xn.p, (size_t)M * d));
    // pointwise_conv1 + GLU in one kernel (round 6): the GEMM runs on the interleaved copy of the weights and its epilogue stores
    // a * sigmoid(b) -- half the bytes written here and read by the depthwise kernel, the gate computed once per element instead
    // of once per staged element (halo rows twice).  Offline bf16 only (the streaming module caches pointwise OUTPUT rows).
    {
      const char* ge = lab_env("RVB_GLU_FUSE");      // read per call: the A/B test flips it inside one process
      const int glu_on = ge ? atoi(ge) : GLU_FUSE_DEFAULT;
      GemmArgs t;
      memset(&t, 0, sizeof(t));
      t.A = e->xn.p; t.W = L.pw1_glu.w.p; t.bias = L.pw1_glu.b.as<float>(); t.C = e->h.p; t.M = M; t.N = 2 * d; t.K = d; t.lda = d; t.ldw = d;
      t.ldc = d; t.alpha = 1.f; t.act = ACT_GLU;
      glu_fused = glu_on && li < 0 && L.pw1_glu.w.p != nullptr && !cal && gemm_glu_supported(e->dtype, t);
      if (glu_fused) {
        Scope sc(e, "gemm", 2.0 * M * (double)t.N * t.K, gemm_alg_bytes(e, t));
        RVB_TRY(gemm(e->stream, e->dtype, t));
        tap_note_gemm(e);
      } else {
        RVB_TRY(run_gemm(e, e->xn.p, d, L.pw1, e->h.p, 2 * d, M, false));
      }
    }
  }
  if (e->tap_live) e->tap_forms[1] = glu_fused ? 1.f : 0.f;
  RVB_TRY(tap_keep(e, "xn_conv", e->xn.p, Md, t16));
  RVB_TRY(tap_keep(e, "glu", e->h.p, glu_fused ? Md : 2 * Md, t16));
  // depthwise conv + LayerNorm + SiLU in one kernel where dwconv_ln() serves the shape: the same bits without the `dconv` tensor.
  // Everything else -- f32, streaming, causal, BatchNorm, fp8 pointwise_conv2, an ungated input, and a tapped block, whose
  // "dconv" tap is that tensor -- runs the two kernels below.
  bool dw_fused = false;
  if (glu_fused && !f8_pw2 && e->cfg.cnn_norm == 0 && !e->cfg.cnn_causal && !e->tap_live) {
    const char* fe = lab_env("RVB_DW_FUSE");       // read per call: the A/B test flips it inside one process
    DwLnArgs g;
    g.G = e->h.p; g.pw1_bias = L.pw1.b.as<float>(); g.dw_w = L.dw_w.as<float>(); g.dw_b = L.dw_b.as<float>(); g.lens = e->cur_lens;
    g.gamma = L.n_cnn.g.as<float>(); g.beta = L.n_cnn.b.as<float>(); g.eps = L.n_cnn.eps; g.out = e->xn.p;
    g.B = B; g.T = T; g.d = d; g.K = e->cfg.cnn_kernel;
    if ((fe ? atoi(fe) : DW_FUSE_DEFAULT) && dwconv_ln_supported(e->dtype, g)) {
      Scope sc(e, "glu_dwconv");
      RVB_TRY(dwconv_ln(e->stream, e->dtype, g));
      dw_fused = true;
    }
  }
  if (!dw_fused) {
    GluDwArgs g;
    g.gated = glu_fused ? 1 : 0;
    g.G = e->h.p; g.pw1_bias = L.pw1.b.as<float>(); g.dw_w = L.dw_w.as<float>(); g.dw_b = L.dw_b.as<float>();
    g.lens = e->cur_lens; g.out = e->dconv.as<float>(); g.B = B; g.T = T; g.d = d; g.K = e->cfg.cnn_kernel;
    g.causal = e->cfg.cnn_causal ? 1 : 0;
    g.out_bf16 = e->dtype == DT_BF16 ? 1 : 0;     // half the bytes to the norm that reads it next (the reference's bf16 autocast rounds here too)
    const int lorder = g.K - 1;
    const bool cached = li >= 0 && g.causal && lorder > 0;
    if (cached) { g.hist = e->stream_st.cnn[li].p; g.hist_rows = e->stream_st.cnn_rows; }
    {
      Scope sc(e, "glu_dwconv");
      RVB_TRY(glu_dwconv(e->stream, e->dtype, g));
    }
    if (cached) {
      // new_cache = cat(cache, x)[:, :, -lorder:] (convolution.py:116-121), kept as pointwise-conv1 OUTPUT rows: that
      // convolution is per frame, so what the reference recomputes from its cached inputs are these very rows
      auto& st = e->stream_st;
      const size_t es = dt_size(e->dtype), rb = (size_t)2 * d * es;
      if (M >= lorder) {
        RVB_HIP_CHECK(hipMemcpyAsync(st.cnn[li].p, (const char*)e->h.p + (size_t)(M - lorder) * rb, (size_t)lorder * rb,
                                     hipMemcpyDeviceToDevice, e->stream));
      } else {
        RVB_HIP_CHECK(hipMemcpyAsync(st.cnn2[li].p, (const char*)st.cnn[li].p + (size_t)M * rb, (size_t)(lorder - M) * rb,
                                     hipMemcpyDeviceToDevice, e->stream));
        RVB_HIP_CHECK(hipMemcpyAsync((char*)st.cnn2[li].p + (size_t)(lorder - M) * rb, e->h.p, (size_t)M * rb,
                                     hipMemcpyDeviceToDevice, e->stream));
        std::swap(st.cnn[li], st.cnn2[li]);
      }
    }
  }
  const int cmode = e->cfg.cnn_norm == 0 ? NORM_LN : NORM_AFFINE;
  const bool dw16 = e->dtype == DT_BF16;
  RVB_TRY(tap_keep(e, "dconv", e->dconv.p, Md, dw16));
  if (f8_pw2) {
    RVB_TRY(run_norm(e, e->dconv.as<float>(), L.n_cnn, e->xn.p, false, M, d, cmode, 1, nullptr, nullptr, nullptr, sc8.in_pw2, 0.f, dw16, satp(4)));
    RVB_TRY(run_gemm8(e, e->xn.p, d, L.pw2, x, d, M, sc8.in_pw2, 1, 1.f, 1.f, ACT_NONE, x, d));
  } else {
    if (!dw_fused) RVB_TRY(run_norm(e, e->dconv.as<float>(), L.n_cnn, e->xn.p, false, M, d, cmode, 1, nullptr, nullptr, nullptr, 0.f, 0.f, dw16));
    RVB_TRY(note(4, e->xn.p, (size_t)M * d));
    RVB_TRY(tap_keep(e, "xn_cnn", e->xn.p, Md, t16));
    RVB_TRY(run_gemm(e, e->xn.p, d, L.pw2, x, d, M, true, 1.f, ACT_NONE, x, d));
  }
  RVB_TRY(tap_keep(e, "x_conv", x, Md, false));
  // feed-forward (+ language-specific mix), final norm     encoder_layer.py:231-244 / :372-402
  if (f8_ff) {
    RVB_TRY(run_norm(e, x, L.n_ff, e->xn.p, false, M, d, NORM_LN, 0, nullptr, nullptr, nullptr, sc8.in_ff1, 0.f, false, satp(5)));
    RVB_TRY(run_gemm8(e, e->xn.p, d, L.ff1, e->h.p, ff, M, sc8.in_ff1, 2, sc8.h_ff, 1.f, ACT_SILU, nullptr, 0, satp(6)));
    RVB_TRY(run_gemm8(e, e->h.p, ff, L.ff2, x, d, M, sc8.h_ff, 1, 1.f, 0.5f, ACT_NONE, x, d));
  } else {
    RVB_TRY(run_norm(e, x, L.n_ff, e->xn.p, false, M, d));
    RVB_TRY(tap_keep(e, "xn_ff", e->xn.p, Md, t16));
    const void* ffin = e->xn.p;
    if (L.is_lsl) {
      RVB_TRY(run_gemm(e, e->xn.p, d, L.lsl, e->y.p, d, M, false));
      RVB_TRY(tap_keep(e, "y", e->y.p, Md, t16));
      ffin = e->y.p;
    } else {
      RVB_TRY(note(5, e->xn.p, (size_t)M * d));
    }
    RVB_TRY(run_gemm(e, ffin, d, L.ff1, e->h.p, ff, M, false, 1.f, ACT_SILU));
    if (!L.is_lsl) RVB_TRY(note(6, e->h.p, (size_t)M * ff));
    RVB_TRY(tap_keep(e, "h_ff", e->h.p, (size_t)M * ff, t16));
    RVB_TRY(run_gemm(e, e->h.p, ff, L.ff2, x, d, M, true, 0.5f, ACT_NONE, x, d));
  }
  RVB_TRY(tap_keep(e, "x_ff", x, Md, false));
  // x = norm_final(x) (+ y for the language-specific block, encoder_layer.py:400), and in the same pass the LayerNorm
  // that always reads it next: the following block's norm_ff_macaron, or the encoder's after_norm (encoder.py:147-148)
  // (the fp8 second output is the NEXT block's in_ffm1: slot 0 of block lidx + 1)
  RVB_TRY(run_norm(e, x, L.n_final, x, true, M, d, NORM_LN, 0, L.is_lsl ? e->y.p : nullptr, &next, next_out, 0.f, f8 ? next8 : 0.f, false,
                   nullptr, (f8 && next8 > 0.f && e->d_f8sat.p) ? e->d_f8sat.as<unsigned>() + (size_t)(lidx + 1) * 8 : nullptr));
  RVB_TRY(tap_keep(e, "x_out", x, Md, false));
  RVB_TRY(tap_keep(e, "next", next_out, Md, t16));
  return OK;
}

int encode_impl(rvb_engine* e, const float* feats, int64_t first_chunk, const int32_t* lens, int B, int T0,
                       int beam, float blank_penalty) {
  const rvb_model_cfg& c = e->cfg;
  if (!e->finalized) { set_error("rvb_encode before rvb_finalize"); return E_STATE; }
  if (B <= 0 || B > c.max_chunks || T0 < 7 || T0 > c.chunk_frames) {
    set_error("rvb_encode: need 1 <= B <= max_chunks and 7 <= T0 <= chunk_frames"); return E_ARG;
  }
  if (beam < 1 || beam > 64 || beam > c.vocab) { set_error("rvb_encode: beam must be in [1,64]"); return E_ARG; }
  // the slices of the sub-batch pipeline (see below)
  int SB = B >= 16 ? (B * 7 + 9) / 10 : B;            // chunks in the first (largest) slice
  if (B >= 64) SB = B - 32;
  if (const char* ov = lab_env("RVB_SLICE0")) { const int v = atoi(ov); if (v > 0 && v <= B) SB = v; }   // tuning override
  if (e->tap_block >= 0 && (SB < B || e->fp8)) {       // refused before anything is touched: the taps hold one slice of a bf16 / f32 pass
    set_error(SB < B ? "rvb_encode: rvb_set_encoder_tap is on, and this batch is encoded in two slices (B >= 16): tap a smaller batch"
                     : "rvb_encode: rvb_set_encoder_tap is on, and the engine runs its fp8 calibration / fp8 pass");
    return E_UNSUPPORTED;
  }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(wait_slices(e, -1));      // a previous batch may still be in flight
  e->stream_st.active = false;      // the offline path reuses the stream's output buffer: an open stream ends here
  const int d = c.d_model, F0 = c.input_dim, V = c.vocab;
  const int T1 = (T0 - 3) / 2 + 1, F1 = (F0 - 3) / 2 + 1, T2 = (T1 - 3) / 2 + 1, F2 = (F1 - 3) / 2 + 1;
  const int M = B * T2;
  const size_t es = dt_size(e->dtype);
  e->B = B; e->T0 = T0; e->T1 = T1; e->F1 = F1; e->T2 = T2; e->F2 = F2; e->beam = beam;
  e->dec_l.kv_ready = e->dec_r.kv_ready = false;
  e->last_blank_penalty = blank_penalty;
  e->in_lens.assign(lens, lens + B);
  e->enc_lens.resize(B);
  std::vector<int32_t> starts(B), qlens(B, T2);
  for (int b = 0; b < B; ++b) {
    if (lens[b] < 0 || lens[b] > T0) { set_error("rvb_encode: lens out of range"); return E_ARG; }
    // mask[:, :, 2::2][:, :, 2::2] (subsampling.py:226): frames 6+4j < len
    e->enc_lens[b] = lens[b] > 6 ? (lens[b] - 7) / 4 + 1 : 0;
    starts[b] = b * T2;
  }
  e->nbest.clear(); e->trie_l.clear(); e->rescored.clear();
  RVB_TRY(upload_i32(e, e->d_enc_lens, e->enc_lens.data(), B));
  RVB_TRY(upload_i32(e, e->d_seq_start, starts.data(), B));
  RVB_TRY(upload_i32(e, e->d_seq_len, qlens.data(), B));

  const float* d_feats;
  if (feats) {
    RVB_TRY(upload_f32(e, e->d_feats_in, feats, (size_t)B * T0 * F0));
    d_feats = e->d_feats_in.as<float>();
  } else {
    const DevBuf& fb = e->packed ? e->feats_packed : e->feats;       // rvb_pause_chunks: the pieces, one per chunk slot
    if (!fb.p || first_chunk < 0 || (first_chunk + B) * (int64_t)T0 > (e->packed ? e->packed_rows : e->feat_rows)) {
      set_error("rvb_encode: device features missing or too short (call rvb_fbank first)"); return E_STATE;
    }
    d_feats = fb.as<float>() + (size_t)first_chunk * T0 * F0;
  }
  // Sub-batch pipeline: the batch is encoded in up to 2 slices on the engine stream; each slice ends with
  // an async D2H copy of its per-frame top-k into pinned memory and an event.  rvb_encode returns once
  // everything is enqueued; the host CTC search of slice i (rvb_ctc_prefix_beam) then runs while the
  // GPU is still encoding slice i+1.  Workspaces are sized for one slice.
  // two slices: with 256x256 GEMM tiles a finer split leaves the N=1024 GEMMs with <2 waves of tiles per CU
  // (measured: 4 slices 818 TFLOP/s vs 923 un-sliced)
  // uneven split: the host search of the LAST slice is the part nothing overlaps, so that slice is the small one;
  // the first slice's search hides under the GPU time of the second.  For large batches the tail is exactly 32
  // chunks (32 x 512 frames = 64 row tiles = one full wave of 256x256 tiles over the 256 CUs for the N = 1024 GEMMs);
  // measured on the 176-chunk bench batch: first slice 96/112/128/144/160 -> 201.1/199.8/198.6/197.4/198.9 ms
  const int Ms = SB * T2;
  RVB_TRY(e->X1.ensure((size_t)SB * T1 * F1 * d * es));
  RVB_TRY(e->X2.ensure((size_t)SB * T2 * F2 * d * es));
  RVB_TRY(e->x.ensure((size_t)Ms * d * 4));
  RVB_TRY(e->xn.ensure((size_t)Ms * d * es));
  RVB_TRY(e->y.ensure((size_t)Ms * d * es));
  RVB_TRY(e->ao.ensure((size_t)Ms * d * es));
  RVB_TRY(e->dconv.ensure((size_t)Ms * d * 4));
  RVB_TRY(e->enc_out.ensure((size_t)M * d * es));
  RVB_TRY(e->h.ensure((size_t)Ms * std::max(c.ffn_dim, 3 * d) * es));
  const int Vld = (V + 3) & ~3;
  RVB_TRY(e->logits.ensure((size_t)LOGIT_SLAB * Vld * 4));
  RVB_TRY(e->topv.ensure((size_t)M * beam * 4));
  RVB_TRY(e->topi.ensure((size_t)M * beam * 4));
  if (e->h_top_cap < (size_t)M * beam) {
    if (e->h_topv) (void)hipHostFree(e->h_topv);
    if (e->h_topi) (void)hipHostFree(e->h_topi);
    e->h_topv = nullptr; e->h_topi = nullptr; e->h_top_cap = 0;
    RVB_HIP_CHECK(hipHostMalloc((void**)&e->h_topv, (size_t)M * beam * 4, hipHostMallocDefault));
    RVB_HIP_CHECK(hipHostMalloc((void**)&e->h_topi, (size_t)M * beam * 4, hipHostMallocDefault));
    e->h_top_cap = (size_t)M * beam;
  }
  e->slices.clear();
  if (e->fp8 && e->f8_state == 0) {     // first batch of an fp8 engine: bf16 pass that records the activation ranges
    RVB_TRY(e->d_amax.ensure((e->enc.size() + 1) * 8 * 4));
    RVB_HIP_CHECK(hipMemsetAsync(e->d_amax.p, 0, (e->enc.size() + 1) * 8 * 4, e->stream));
    RVB_TRY(reset_f8sat(e));
    e->f8_state = 1;
  }
  for (int c0 = 0; c0 < B; c0 += SB) {
    const int nb = std::min(SB, B - c0);               // first slice SB chunks, second slice the rest (<= SB)
    const int m = nb * T2;
    const int row0 = c0 * T2;
    e->cur_lens = e->d_enc_lens.as<int>() + c0;       // per-chunk arrays of this slice (starts are slice-relative)
    // Conv2dSubsampling4 (subsampling.py:201-226): cmvn+conv1 -> conv2 (implicit GEMM) -> linear * sqrt(d)
    // fp8 mode with conv2 in the policy (bit 5): conv1 writes e4m3 at the calibrated scale and conv2 runs on the fp8 phase loop
    const bool f8c2 = e->fp8 && e->f8_state == 2 && e->f8_conv2 && e->f8_x1 > 0.f && e->conv2.w8.p && d % 128 == 0;
    const bool calx = e->fp8 && e->f8_state == 1;
    struct TapLive { rvb_engine* e; ~TapLive() { e->tap_live = false; } } tap_guard{e};
    e->tap_live = e->tap_block == (int)e->enc.size();       // the front end's taps (rvb_set_encoder_tap)
    if (e->tap_live) e->tap_forms.clear();
    const bool t16 = e->dtype == DT_BF16;
    {
      Scope sc(e, "subsample");
      RVB_TRY(subsample_conv1(e->stream, e->dtype, d_feats + (size_t)c0 * T0 * F0, e->cmvn_mean.as<float>(),
                              e->cmvn_istd.as<float>(), e->conv1_w.as<float>(), e->conv1_b.as<float>(), e->X1.p, nb, T0, F0, d,
                              f8c2 ? e->f8_x1 : 0.f, calx ? e->d_amax.as<unsigned>() + e->enc.size() * 8 : nullptr,
                              (f8c2 && e->d_f8sat.p) ? e->d_f8sat.as<unsigned>() + e->enc.size() * 8 + 1 : nullptr));
    }
    {
      GemmArgs g;
      memset(&g, 0, sizeof(g));
      g.A = e->X1.p; g.W = e->conv2.w.p; g.bias = e->conv2.b.as<float>(); g.C = e->X2.p;
      g.M = nb * T2 * F2; g.N = d; g.K = 9 * d; g.lda = d; g.ldw = 9 * d; g.ldc = d;
      g.alpha = 1.f; g.act = ACT_RELU; g.conv = 1; g.cT1 = T1; g.cF1 = F1; g.cT2 = T2; g.cF2 = F2; g.cC = d;
      if (f8c2) { g.W = e->conv2.w8.p; g.in_fp8 = 1; g.a_scale = e->f8_x1; g.w_scale = e->conv2.wscale.as<float>(); }
      Scope sc(e, f8c2 ? "gemm_fp8" : "gemm", 2.0 * g.M * (double)g.N * g.K, gemm_alg_bytes(e, g));
      RVB_TRY(gemm(e->stream, e->dtype, g));
      tap_note_gemm(e);
    }
    RVB_TRY(tap_keep(e, "X1", e->X1.p, (size_t)nb * T1 * F1 * d, t16));
    RVB_TRY(tap_keep(e, "X2", e->X2.p, (size_t)m * F2 * d, t16));
    RVB_TRY(run_gemm(e, e->X2.p, F2 * d, e->embed_out, e->x.p, d, m, true, std::sqrt((float)d)));
    RVB_TRY(tap_keep(e, "x0", e->x.p, (size_t)m * d, false));
    void* eo = (char*)e->enc_out.p + (size_t)row0 * d * es;
    const bool f8 = e->fp8 && e->f8_state == 2;
    RVB_TRY(run_norm(e, e->x.as<float>(), e->enc[0].n_ffm, e->xn.p, false, m, d, NORM_LN, 0, nullptr, nullptr, nullptr,
                     (f8 && (e->f8_groups[0] & 1u)) ? e->f8[0].in_ffm1 : 0.f, 0.f, false, e->d_f8sat.as<unsigned>()));
    RVB_TRY(tap_keep(e, "xn0", e->xn.p, (size_t)m * d, t16));
    e->tap_live = false;
    for (size_t li = 0; li < e->enc.size(); ++li) {
      const bool last = li + 1 == e->enc.size();
      RVB_TRY(encoder_layer(e, e->enc[li], (int)li, m, nb, T2, last ? e->enc_after : e->enc[li + 1].n_ffm, last ? eo : e->xn.p,
                            (f8 && !last && (e->f8_groups[li + 1] & 1u)) ? e->f8[li + 1].in_ffm1 : 0.f));
    }
    // CTC head + log-softmax + per-frame top-k (ctc.py:106-114, search.py:155)
    for (int r0 = 0; r0 < m; r0 += LOGIT_SLAB) {
      const int rows = std::min(LOGIT_SLAB, m - r0);
      RVB_TRY(run_gemm(e, (const char*)eo + (size_t)r0 * d * es, d, e->ctc, e->logits.p, Vld, rows, true));
      Scope sc(e, "ctc_topk");
      RVB_TRY(logsoftmax_topk(e->stream, e->logits.as<float>(), rows, V, Vld, beam, blank_penalty, c.blank_id,
                              e->topv.as<float>() + (size_t)(row0 + r0) * beam, e->topi.as<int>() + (size_t)(row0 + r0) * beam, nullptr));
    }
    RVB_HIP_CHECK(hipMemcpyAsync(e->h_topv + (size_t)row0 * beam, e->topv.as<float>() + (size_t)row0 * beam, (size_t)m * beam * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipMemcpyAsync(e->h_topi + (size_t)row0 * beam, e->topi.as<int>() + (size_t)row0 * beam, (size_t)m * beam * 4, hipMemcpyDeviceToHost, e->stream));
    hipEvent_t ev;
    if (!e->slice_event_pool.empty()) { ev = e->slice_event_pool.back(); e->slice_event_pool.pop_back(); }
    else RVB_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    RVB_HIP_CHECK(hipEventRecord(ev, e->stream));
    e->slices.push_back({c0, nb, ev, false});
  }
  if (e->f8_state == 1) {
    // per-tensor scales: a power of two with headroom (2 * amax maps inside +-448; fp8 is floating point, so headroom
    // costs no relative precision); later batches saturate only beyond twice the calibration batch's maximum
    std::vector<float> am((e->enc.size() + 1) * 8);
    RVB_HIP_CHECK(hipMemcpyAsync(am.data(), e->d_amax.p, am.size() * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    e->f8.resize(e->enc.size());
    auto sc = [](float a) { return a > 0.f ? std::exp2(std::ceil(std::log2(2.f * a / 448.f))) : 1.f; };
    for (size_t l = 0; l < e->enc.size(); ++l) {
      const float* a = am.data() + l * 8;
      e->f8[l] = {sc(a[0]), sc(a[1]), sc(a[2]), sc(a[3]), sc(a[4]), sc(a[5]), sc(a[6])};
    }
    e->f8_x1 = am[e->enc.size() * 8] > 0.f ? sc(am[e->enc.size() * 8]) : 0.f;       // conv1's output (>= 0: the float bits were max'ed as unsigned)
    if (e->f8_groups.size() != e->enc.size()) RVB_TRY(set_fp8_policy_impl(e, -1, 0, -1));     // default policy (or RVB_FP8_*)
    e->f8_state = 2;
  }
  return OK;
}

// wait until slice `i` (or every slice when i < 0) of the last rvb_encode has reached the host
int wait_slices(rvb_engine* e, int i) {
  for (size_t k = 0; k < e->slices.size(); ++k) {
    if (i >= 0 && (int)k != i) continue;
    auto& sl = e->slices[k];
    if (sl.done) continue;
    RVB_HIP_CHECK(hipEventSynchronize(sl.ev));
    e->slice_event_pool.push_back(sl.ev);
    sl.done = true;
  }
  return OK;
}

// ------------------------------------------------------------------------------------ streaming encoder
// BaseEncoder.forward_chunk / forward_chunk_by_chunk (encoder.py:231-402) for one stream: the attention cache (keys
// and values of the frames already seen, per layer) lives in the engine; the reference hands it back and forth as
// a tensor.  Non-causal convolution modules carry no cnn cache (lorder = 0, convolution.py:118-123): the depthwise
// convolution sees zeros beyond the chunk, exactly as the reference's Conv1d padding does.  Causal ones (cnn_causal)
// keep, per block, the pointwise-conv1 outputs of the last K-1 frames (encoder_layer() below).
int stream_begin_impl(rvb_engine* e) {
  if (!e->finalized) { set_error("rvb_stream_begin before rvb_finalize"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(wait_slices(e, -1));
  const int d = e->cfg.d_model;
  const size_t es = dt_size(e->dtype);
  auto& st = e->stream_st;
  st.kv.resize(e->enc.size()); st.kv2.resize(e->enc.size());
  for (size_t l = 0; l < e->enc.size(); ++l) {
    RVB_TRY(st.kv[l].ensure((size_t)e->pe_rows * 2 * d * es));
    RVB_TRY(st.kv2[l].ensure((size_t)e->pe_rows * 2 * d * es));
  }
  RVB_TRY(e->enc_out.ensure((size_t)e->pe_rows * d * es));
  if (e->cfg.cnn_causal && e->cfg.cnn_kernel > 1) {
    st.cnn.resize(e->enc.size()); st.cnn2.resize(e->enc.size());
    for (size_t l = 0; l < e->enc.size(); ++l) {
      RVB_TRY(st.cnn[l].ensure((size_t)(e->cfg.cnn_kernel - 1) * 2 * d * es));
      RVB_TRY(st.cnn2[l].ensure((size_t)(e->cfg.cnn_kernel - 1) * 2 * d * es));
    }
  }
  st.active = true; st.offset = 0; st.cache_len = 0; st.cnn_rows = 0;
  e->B = 0; e->nbest.clear(); e->trie_l.clear(); e->rescored.clear(); e->slices.clear();
  e->dec_l.kv_ready = e->dec_r.kv_ready = false;
  return OK;
}

int stream_chunk_impl(rvb_engine* e, const float* feats, int T0, int required_cache_size, float* out, int32_t* n_out) {
  const rvb_model_cfg& c = e->cfg;
  auto& st = e->stream_st;
  if (!st.active) { set_error("rvb_stream_chunk before rvb_stream_begin"); return E_STATE; }
  if (T0 < 7) { set_error("rvb_stream_chunk: a chunk needs at least 7 input frames (Conv2dSubsampling4)"); return E_ARG; }
  if (e->tap_block >= 0) { set_error("rvb_stream_chunk: rvb_set_encoder_tap is on (the taps are the offline encoder's)"); return E_UNSUPPORTED; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  const int d = c.d_model, F0 = c.input_dim;
  const int T1 = (T0 - 3) / 2 + 1, F1 = (F0 - 3) / 2 + 1, T2 = (T1 - 3) / 2 + 1, F2 = (F1 - 3) / 2 + 1;
  const int M = T2;
  const size_t es = dt_size(e->dtype);
  if (st.offset + M > e->pe_rows) {
    set_error("rvb_stream_chunk: more than " + std::to_string(e->pe_rows) + " encoder frames in one stream (the reference's positional "
              "table has max_len 5000 rows, embedding.py:33)");
    return E_UNSUPPORTED;
  }
  RVB_TRY(e->X1.ensure((size_t)T1 * F1 * d * es));
  RVB_TRY(e->X2.ensure((size_t)T2 * F2 * d * es));
  RVB_TRY(e->x.ensure((size_t)M * d * 4));
  RVB_TRY(e->xn.ensure((size_t)M * d * es));
  RVB_TRY(e->y.ensure((size_t)M * d * es));
  RVB_TRY(e->ao.ensure((size_t)M * d * es));
  RVB_TRY(e->dconv.ensure((size_t)M * d * 4));
  RVB_TRY(e->h.ensure((size_t)M * std::max(c.ffn_dim, 3 * d) * es));
  RVB_TRY(upload_f32(e, e->d_feats_in, feats, (size_t)T0 * F0));
  const int32_t zero = 0, mm = M, kv[2] = {0, st.cache_len + M};
  RVB_TRY(upload_i32(e, e->d_seq_start, &zero, 1));
  RVB_TRY(upload_i32(e, e->d_seq_len, &mm, 1));
  RVB_TRY(upload_i32(e, e->d_enc_lens, &mm, 1));
  RVB_TRY(upload_i32(e, e->d_stream_i32, kv, 2));
  e->cur_lens = e->d_enc_lens.as<int>();
  {
    Scope sc(e, "subsample");
    RVB_TRY(subsample_conv1(e->stream, e->dtype, e->d_feats_in.as<float>(), e->cmvn_mean.as<float>(), e->cmvn_istd.as<float>(),
                            e->conv1_w.as<float>(), e->conv1_b.as<float>(), e->X1.p, 1, T0, F0, d));
  }
  {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = e->X1.p; g.W = e->conv2.w.p; g.bias = e->conv2.b.as<float>(); g.C = e->X2.p;
    g.M = T2 * F2; g.N = d; g.K = 9 * d; g.lda = d; g.ldw = 9 * d; g.ldc = d;
    g.alpha = 1.f; g.act = ACT_RELU; g.conv = 1; g.cT1 = T1; g.cF1 = F1; g.cT2 = T2; g.cF2 = F2; g.cC = d;
    Scope sc(e, "gemm", 2.0 * g.M * (double)g.N * g.K, gemm_alg_bytes(e, g));
    RVB_TRY(gemm(e->stream, e->dtype, g));
  }
  RVB_TRY(run_gemm(e, e->X2.p, F2 * d, e->embed_out, e->x.p, d, M, true, std::sqrt((float)d)));
  void* eo = (char*)e->enc_out.p + (size_t)st.offset * d * es;
  RVB_TRY(run_norm(e, e->x.as<float>(), e->enc[0].n_ffm, e->xn.p, false, M, d));
  for (size_t li = 0; li < e->enc.size(); ++li) {
    const bool last = li + 1 == e->enc.size();
    RVB_TRY(encoder_layer(e, e->enc[li], (int)li, M, 1, M, last ? e->enc_after : e->enc[li + 1].n_ffm, last ? eo : e->xn.p, 0.f, (int)li));
  }
  if (out) {
    if (e->dtype == DT_F32) {
      RVB_HIP_CHECK(hipMemcpyAsync(out, eo, (size_t)M * d * 4, hipMemcpyDeviceToHost, e->stream));
      RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    } else {
      std::vector<bf16_t> tmp((size_t)M * d);
      RVB_HIP_CHECK(hipMemcpyAsync(tmp.data(), eo, tmp.size() * 2, hipMemcpyDeviceToHost, e->stream));
      RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
      for (size_t i = 0; i < tmp.size(); ++i) out[i] = bf16_to_f32(tmp[i]);
    }
  }
  // r_att_cache = new_att_cache[:, :, next_cache_start:, :] (encoder.py:307-312,331)
  const int key_size = st.cache_len + M;
  int start = 0;
  if (required_cache_size == 0) start = key_size;
  else if (required_cache_size > 0) start = std::max(key_size - required_cache_size, 0);
  const int keep = key_size - start;
  if (start > 0 && keep > 0) {
    for (size_t l = 0; l < e->enc.size(); ++l) {
      RVB_HIP_CHECK(hipMemcpyAsync(st.kv2[l].p, (const char*)st.kv[l].p + (size_t)start * 2 * d * es, (size_t)keep * 2 * d * es,
                                   hipMemcpyDeviceToDevice, e->stream));
      std::swap(st.kv[l], st.kv2[l]);
    }
  }
  st.cache_len = keep;
  st.cnn_rows = std::min(st.cnn_rows + M, std::max(c.cnn_kernel - 1, 0));
  st.offset += M;
  if (n_out) *n_out = M;
  return OK;
}

// CTC head + top-k over everything the stream produced: from here on the stream is one encoded "chunk" of st.offset
// frames and the search entry points work on it (ASRModel._forward_encoder with simulate_streaming, asr_model.py:301-306)
int stream_finish_impl(rvb_engine* e, int beam, float blank_penalty) {
  const rvb_model_cfg& c = e->cfg;
  auto& st = e->stream_st;
  if (!st.active) { set_error("rvb_stream_finish before rvb_stream_begin"); return E_STATE; }
  if (beam < 1 || beam > 64 || beam > c.vocab) { set_error("rvb_stream_finish: beam must be in [1,64]"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  const int d = c.d_model, V = c.vocab, M = st.offset;
  const size_t es = dt_size(e->dtype);
  if (M <= 0) { set_error("rvb_stream_finish: the stream produced no encoder frame"); return E_STATE; }
  e->B = 1; e->T2 = M; e->beam = beam; e->T0 = 0;
  e->dec_l.kv_ready = e->dec_r.kv_ready = false;
  e->last_blank_penalty = blank_penalty;
  e->in_lens.assign(1, 0); e->enc_lens.assign(1, M);
  e->nbest.clear(); e->trie_l.clear(); e->rescored.clear();
  const int Vld = (V + 3) & ~3;
  RVB_TRY(e->logits.ensure((size_t)LOGIT_SLAB * Vld * 4));
  RVB_TRY(e->topv.ensure((size_t)M * beam * 4));
  RVB_TRY(e->topi.ensure((size_t)M * beam * 4));
  if (e->h_top_cap < (size_t)M * beam) {
    if (e->h_topv) (void)hipHostFree(e->h_topv);
    if (e->h_topi) (void)hipHostFree(e->h_topi);
    e->h_topv = nullptr; e->h_topi = nullptr; e->h_top_cap = 0;
    RVB_HIP_CHECK(hipHostMalloc((void**)&e->h_topv, (size_t)M * beam * 4, hipHostMallocDefault));
    RVB_HIP_CHECK(hipHostMalloc((void**)&e->h_topi, (size_t)M * beam * 4, hipHostMallocDefault));
    e->h_top_cap = (size_t)M * beam;
  }
  for (int r0 = 0; r0 < M; r0 += LOGIT_SLAB) {
    const int rows = std::min(LOGIT_SLAB, M - r0);
    RVB_TRY(run_gemm(e, (const char*)e->enc_out.p + (size_t)r0 * d * es, d, e->ctc, e->logits.p, Vld, rows, true));
    Scope sc(e, "ctc_topk");
    RVB_TRY(logsoftmax_topk(e->stream, e->logits.as<float>(), rows, V, Vld, beam, blank_penalty, c.blank_id,
                            e->topv.as<float>() + (size_t)r0 * beam, e->topi.as<int>() + (size_t)r0 * beam, nullptr));
  }
  RVB_HIP_CHECK(hipMemcpyAsync(e->h_topv, e->topv.p, (size_t)M * beam * 4, hipMemcpyDeviceToHost, e->stream));
  RVB_HIP_CHECK(hipMemcpyAsync(e->h_topi, e->topi.p, (size_t)M * beam * 4, hipMemcpyDeviceToHost, e->stream));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->slices.clear();
  e->slices.push_back({0, 1, nullptr, true});
  st.active = false;
  return OK;
}

}  // namespace rvb
