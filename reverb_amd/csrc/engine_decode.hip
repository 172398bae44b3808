// librvb engine, decoding: the CTC prefix beam search's host glue, the rescoring trie and decoder (rvb_attention_rescore,
// rvb_attention_score), the attention beam search and joint_decoding.
#include "engine_impl.h"
#include "trie.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace rvb {

// ------------------------------------------------------------------------------------ search
// Host threads one engine may use for the search: RVB_SEARCH_THREADS, else this process's share of the cores when
// several ranks run on the node (LOCAL_WORLD_SIZE is set by torchrun), at most 32.
static unsigned search_threads() {
  if (const char* s = getenv("RVB_SEARCH_THREADS")) {
    const int v = atoi(s);
    if (v > 0) return (unsigned)v;
  }
  unsigned hw = std::thread::hardware_concurrency();
  if (hw == 0) hw = 4;
  if (const char* s = getenv("LOCAL_WORLD_SIZE")) {
    const int v = atoi(s);
    if (v > 1) hw = std::max(1u, hw / (unsigned)v);
  }
  return std::min(hw, 32u);
}

static void build_chunk_trie(rvb_engine* e, int b, bool reversed, int sos, int eos, TrieBatch* t);   // with the rescoring, below

int prefix_beam_impl(rvb_engine* e, int beam) {
  if (e->B <= 0) { set_error("rvb_ctc_prefix_beam before rvb_encode"); return E_STATE; }
  // the search beam may be narrower than the top-k rvb_encode kept per frame (joint_decoding's pre-beam needs more): the first
  // `beam` entries of a frame's descending top-k ARE its top-`beam` (search.py:155 `logp.topk(beam_size)`)
  if (beam < 1 || beam > e->beam) { set_error("rvb_ctc_prefix_beam: beam exceeds the top-k kept by rvb_encode"); return E_ARG; }
  const int B = e->B, T = e->T2, K = e->beam;
  e->nbest.assign(B, PrefixResult());
  const bool prebuild = e->dec_l.present;
  e->trie_l.assign(prebuild ? B : 0, TrieBatch());
  const unsigned hw = search_threads();
  double busy_ms = 0.0;
  for (size_t si = 0; si < e->slices.size(); ++si) {
    RVB_TRY(wait_slices(e, (int)si));            // GPU keeps encoding the later slices meanwhile
    const auto t0 = std::chrono::steady_clock::now();
    const int c0 = e->slices[si].c0, nb = e->slices[si].nb;
    // ~0.5 ms of work per full chunk: two or more chunks per thread amortise the thread start; chunks are handed
    // out one at a time because their lengths (and so their cost) differ
    const unsigned nthr = std::max(1u, std::min<unsigned>(hw, (unsigned)(nb + 1) / 2));
    std::atomic<int> next_chunk(c0);
    const int sos = e->cfg.sos_id, eos = e->cfg.eos_id;
    const ContextGraph* graph = e->context_graph.get();   // read-only, shared by the workers
    auto work = [&, c0, nb]() {
      for (int b = next_chunk.fetch_add(1); b < c0 + nb; b = next_chunk.fetch_add(1)) {
        prefix_beam_search(e->h_topv + (size_t)b * T * K, e->h_topi + (size_t)b * T * K, e->enc_lens[b], K,
                           beam, e->cfg.blank_id, &e->nbest[b], graph);
        // the chunk's prefix trie for the left-to-right rescoring decoder, while the worker has the n-best list hot: for
        // every slice but the last this happens underneath the encoder of the next slice (rescore_impl only stitches)
        if (prebuild) build_chunk_trie(e, b, false, sos, eos, &e->trie_l[b]);
      }
    };
    e->pool.run(nthr, work);                     // the calling thread is one of the nthr
    busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  auto& pe = e->prof["search_host"];
  pe.ms += busy_ms;
  pe.launches += 1;
  return OK;
}

// ------------------------------------------------------------------------------------ rescoring
// the trie of a batch's distinct prefixes, one decoder row each: trie.h (build_trie_range, merge_tries)

// one decoder over the trie rows; logp[slot] = log p(target | prefix) for every ask (TrieBatch::pair_slot maps pairs)
// One chunk's trie in local numbering (rows, hypotheses, path entries and pairs counted from 0).
static void build_chunk_trie(rvb_engine* e, int b, bool reversed, int sos, int eos, TrieBatch* t) {
  const PrefixResult& pr = e->nbest[b];
  std::vector<HypRef> hyps(pr.nbest.size());
  for (size_t i = 0; i < hyps.size(); ++i) hyps[i] = {b, (int)i, (int)pr.nbest[i].size(), 0};
  if (reversed)
    build_trie_range(hyps.data(), hyps.data() + hyps.size(), b, 1, sos, eos,
                     [&](const HypRef& h, int j) { return pr.nbest[h.idx][h.len - 1 - j]; }, t);
  else
    build_trie_range(hyps.data(), hyps.data() + hyps.size(), b, 1, sos, eos, [&](const HypRef& h, int j) { return pr.nbest[h.idx][j]; }, t);
}

// every chunk's trie on the host pool, then stitched
static void build_trie_parallel(rvb_engine* e, bool reversed, TrieBatch* t) {
  const int B = e->B, sos = e->cfg.sos_id, eos = e->cfg.eos_id;
  std::vector<TrieBatch> part(B);
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) build_chunk_trie(e, b, reversed, sos, eos, &part[b]);
  };
  e->pool.run(std::max(1u, std::min<unsigned>(search_threads(), (unsigned)B / 4)), work);
  merge_tries(part, t);
}

// Keys / values of the encoder output for every decoder layer (decoder_layer.py:112-119: `src_attn(x, memory, memory)`; the
// reference projects the memory once per hypothesis, asr_model.py:895): they depend on the encoder output alone, so they can
// be enqueued before the CTC search of the last slice has produced a single hypothesis (rvb_prepare_rescoring) -- the device
// computes them while the host searches.
int decoder_memory_kv(rvb_engine* e, Decoder& D, int M) {
  const int d = e->cfg.d_model;
  const size_t es = dt_size(e->dtype);
  for (auto& L : D.layers) {
    RVB_TRY(L.kvmem.ensure((size_t)M * 2 * d * es));
    RVB_TRY(run_gemm(e, e->enc_out.p, d, L.src_kv, L.kvmem.p, 2 * d, M, false));
  }
  D.kv_ready = true;
  return OK;
}

// xent (rvb_attention_score): the slabs go through row_xent instead of lse_gather_multi, which also returns lse, the sum of the
// logits and the arg-max of every trie row; null (rescoring): the launches are exactly the ones they always were
struct XentRows { std::vector<float> lse; std::vector<double> sum_x; std::vector<int32_t> top1; };
// Decoder taps (rvb_set_decoder_tap): while a tapped decoder_forward runs, the decoder's map and forms stand in for the encoder's, so
// tap_keep / tap_note_gemm / tap_note_attention write there; e->tap_live is raised inside the tapped position only.  Off: nothing.
struct DecTapScope {
  rvb_engine* e; bool on;
  DecTapScope(rvb_engine* e_, bool on_) : e(e_), on(on_) {
    if (!on) return;
    std::swap(e->taps, e->dtaps); std::swap(e->tap_forms, e->dtap_forms);
    e->tap_forms.clear(); e->dtap_trie.clear();
  }
  ~DecTapScope() {
    if (!on) return;
    e->tap_live = false;
    std::swap(e->taps, e->dtaps); std::swap(e->tap_forms, e->dtap_forms);
  }
};
static int decoder_forward(rvb_engine* e, Decoder& D, const TrieBatch& t, std::vector<float>* logp, XentRows* xent = nullptr) {
  const rvb_model_cfg& c = e->cfg;
  const int d = c.d_model, heads = c.dec_heads, dk = d / heads, ff = c.dec_ffn_dim, V = c.vocab;
  const int M = e->B * e->T2, R = t.R, nhyp = (int)t.hq_start.size();
  const size_t es = dt_size(e->dtype);
  const int nlayers = (int)D.layers.size();
  const int tap_pos = e->dtap_pos >= 0 && &D == (e->dtap_side ? &e->dec_r : &e->dec_l) ? e->dtap_pos : -1;
  const bool t16 = e->dtype == DT_BF16;
  DecTapScope taps(e, tap_pos >= 0);
  if (tap_pos >= 0) {       // the batch as the host built it: [13, the 13 lengths, the arrays], int32 carried in floats
    const std::vector<int32_t>* arr[13] = {&t.tok, &t.pos, &t.path, &t.hq_start, &t.hq_len, &t.hq_pos0, &t.hkv_start, &t.hkv_len,
                                           &t.crow_start, &t.crow_len, &t.tgt_ptr, &t.tgt, &t.work};
    e->dtap_trie.push_back(13.f);
    for (auto* a : arr) e->dtap_trie.push_back((float)a->size());
    for (auto* a : arr) for (int32_t v : *a) e->dtap_trie.push_back((float)v);
    e->dtap_rows = R;
  }
  RVB_TRY(upload_i32(e, e->d_tok, t.tok.data(), R));
  RVB_TRY(upload_i32(e, e->d_pos, t.pos.data(), R));
  RVB_TRY(upload_i32(e, e->d_tgt, t.tgt.data(), t.P));
  RVB_TRY(upload_i32(e, e->d_tgt_ptr, t.tgt_ptr.data(), R + 1));
  RVB_TRY(upload_i32(e, e->d_path, t.path.data(), t.path.size()));
  RVB_TRY(upload_i32(e, e->d_work, t.work.data(), t.work.size()));
  RVB_TRY(upload_i32(e, e->d_hq_start, t.hq_start.data(), nhyp));
  RVB_TRY(upload_i32(e, e->d_hq_len, t.hq_len.data(), nhyp));
  RVB_TRY(upload_i32(e, e->d_hq_pos0, t.hq_pos0.data(), nhyp));
  RVB_TRY(upload_i32(e, e->d_hpath_start, t.hkv_start.data(), nhyp));
  RVB_TRY(upload_i32(e, e->d_hpath_len, t.hkv_len.data(), nhyp));
  RVB_TRY(upload_i32(e, e->d_hkv_start, t.crow_start.data(), e->B));
  RVB_TRY(upload_i32(e, e->d_hkv_len, t.crow_len.data(), e->B));
  RVB_TRY(e->dx.ensure((size_t)R * d * 4));
  RVB_TRY(e->dxn.ensure((size_t)R * d * es));
  RVB_TRY(e->dy.ensure((size_t)R * d * es));
  RVB_TRY(e->dao.ensure((size_t)R * d * es));
  RVB_TRY(e->dq.ensure((size_t)R * d * es));
  RVB_TRY(e->dqkv.ensure((size_t)R * 3 * d * es));
  RVB_TRY(e->dh.ensure((size_t)R * ff * es));
  if (!D.kv_ready) RVB_TRY(decoder_memory_kv(e, D, M));
  RVB_TRY(e->d_logp.ensure((size_t)t.P * 4));
  if (xent) {
    RVB_TRY(e->d_xlse.ensure((size_t)R * 4)); RVB_TRY(e->d_xsum.ensure((size_t)R * 8)); RVB_TRY(e->d_xtop.ensure((size_t)R * 4));
  }
  float* x = e->dx.as<float>();
  {
    Scope sc(e, "embed");
    RVB_TRY(embed_tokens(e->stream, D.embed.as<float>(), e->pe_f32.as<float>(), e->d_tok.as<int>(), e->d_pos.as<int>(),
                         x, R, d, std::sqrt((float)d)));
  }
  const size_t Rd = (size_t)R * d;
  for (int li = 0; li < nlayers; ++li) {
    DecLayer& L = D.layers[li];
    e->tap_live = li == tap_pos;
    if (li == 0) RVB_TRY(tap_keep(e, "x_emb", x, Rd, false));
    RVB_TRY(tap_keep(e, "x_in", x, Rd, false));
    RVB_TRY(tap_keep(e, "kvmem", L.kvmem.p, (size_t)M * 2 * d, t16));
    // self attention (causal): a hypothesis' owned rows are the queries, the rows of its whole prefix path the keys
    // decoder_layer.py:91-110, decoder.py:150-156
    RVB_TRY(run_norm(e, x, L.n1, e->dxn.p, false, R, d));
    RVB_TRY(tap_keep(e, "xn1", e->dxn.p, Rd, t16));
    RVB_TRY(run_gemm(e, e->dxn.p, d, L.self_qkv, e->dqkv.p, 3 * d, R, false));
    RVB_TRY(tap_keep(e, "qkv", e->dqkv.p, 3 * Rd, t16));
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = e->dqkv.p; a.k = (const char*)e->dqkv.p + (size_t)d * es; a.v = (const char*)e->dqkv.p + (size_t)2 * d * es;
    a.q_stride = a.k_stride = a.v_stride = 3 * d; a.o_stride = d; a.out = e->dao.p;
    a.q_start = e->d_hq_start.as<int>(); a.q_len = e->d_hq_len.as<int>(); a.q_pos0 = e->d_hq_pos0.as<int>();
    a.kv_start = e->d_hpath_start.as<int>(); a.kv_len = e->d_hpath_len.as<int>(); a.kv_index = e->d_path.as<int>();
    a.work = e->d_work.as<int>(); a.n_work = (int)t.work.size() / 2; a.q_block = 16;
    a.nseq = nhyp; a.heads = heads; a.dk = dk; a.max_q = 16; a.causal = 1; a.sqrt_dk = std::sqrt((float)dk);
    {
      Scope sc(e, "attention");
      RVB_TRY(attention(e->stream, e->dtype, with_lab(a)));
      tap_note_attention(e);
    }
    RVB_TRY(tap_keep(e, "ao_self", e->dao.p, Rd, t16));
    RVB_TRY(run_gemm(e, e->dao.p, d, L.self_out, x, d, R, true, 1.f, ACT_NONE, x, d));
    RVB_TRY(tap_keep(e, "x_self", x, Rd, false));
    // cross attention over the chunk's encoder frames (memory K/V computed once, not per hypothesis:
    // the reference repeats the memory N times, asr_model.py:895)       decoder_layer.py:112-119
    RVB_TRY(run_norm(e, x, L.n2, e->dxn.p, false, R, d));
    RVB_TRY(tap_keep(e, "xn2", e->dxn.p, Rd, t16));
    RVB_TRY(run_gemm(e, e->dxn.p, d, L.src_q, e->dq.p, d, R, false));
    RVB_TRY(tap_keep(e, "q", e->dq.p, Rd, t16));
    memset(&a, 0, sizeof(a));
    a.q = e->dq.p; a.k = L.kvmem.p; a.v = (const char*)L.kvmem.p + (size_t)d * es;
    a.q_stride = d; a.k_stride = a.v_stride = 2 * d; a.o_stride = d; a.out = e->dao.p;
    // all rows of a chunk attend to the same memory and there is no causal mask: they form ONE query sequence per
    // chunk, so the chunk's K/V tiles are staged once per 128 rows
    a.q_start = e->d_hkv_start.as<int>(); a.q_len = e->d_hkv_len.as<int>();
    a.kv_start = e->d_aux_i32.as<int>(); a.kv_len = e->d_aux_i32.as<int>() + e->B;
    a.nseq = e->B; a.heads = heads; a.dk = dk; a.max_q = t.max_chunk_rows; a.causal = 0; a.sqrt_dk = std::sqrt((float)dk);
    {
      Scope sc(e, "attention");
      RVB_TRY(attention(e->stream, e->dtype, with_lab(a)));
      tap_note_attention(e);
    }
    RVB_TRY(tap_keep(e, "ao_src", e->dao.p, Rd, t16));
    RVB_TRY(run_gemm(e, e->dao.p, d, L.src_out, x, d, R, true, 1.f, ACT_NONE, x, d));
    RVB_TRY(tap_keep(e, "x_src", x, Rd, false));
    // feed forward (ReLU) with the language-specific mix     decoder_layer.py:121-127 / :313-333
    RVB_TRY(run_norm(e, x, L.n3, e->dxn.p, false, R, d));
    RVB_TRY(tap_keep(e, "xn3", e->dxn.p, Rd, t16));
    const void* ffin = e->dxn.p;
    if (L.is_lsl) {
      RVB_TRY(run_gemm(e, e->dxn.p, d, L.lsl, e->dy.p, d, R, false));
      RVB_TRY(tap_keep(e, "y", e->dy.p, Rd, t16));
      ffin = e->dy.p;
    }
    RVB_TRY(run_gemm(e, ffin, d, L.ff1, e->dh.p, ff, R, false, 1.f, ACT_RELU));
    RVB_TRY(tap_keep(e, "h", e->dh.p, (size_t)R * ff, t16));
    RVB_TRY(run_gemm(e, e->dh.p, ff, L.ff2, x, d, R, true, 1.f, ACT_NONE, x, d));
    RVB_TRY(tap_keep(e, "x_ff", x, Rd, false));
  }
  e->tap_live = tap_pos == nlayers;
  RVB_TRY(tap_keep(e, "x_in", x, Rd, false));
  RVB_TRY(run_norm(e, x, D.after, e->dxn.p, false, R, d));
  RVB_TRY(tap_keep(e, "xn_after", e->dxn.p, Rd, t16));
  const int Vld = (V + 3) & ~3;
  if (e->tap_live && R > LOGIT_SLAB) {       // the logits exist one slab at a time: none is kept, and rvb_get_decoder_tap says so
    auto it = e->taps.find("logits");
    if (it != e->taps.end()) { it->second.buf.release(); e->taps.erase(it); }
  }
  for (int r0 = 0; r0 < R; r0 += LOGIT_SLAB) {
    const int rows = std::min(LOGIT_SLAB, R - r0);
    RVB_TRY(run_gemm(e, (const char*)e->dxn.p + (size_t)r0 * d * es, d, D.out, e->logits.p, Vld, rows, true));
    if (R <= LOGIT_SLAB) RVB_TRY(tap_keep(e, "logits", e->logits.p, (size_t)R * Vld, false));
    Scope sc(e, "lse_gather");
    if (xent)
      RVB_TRY(row_xent(e->stream, e->logits.as<float>(), rows, V, Vld, e->d_tgt_ptr.as<int>() + r0, e->d_tgt.as<int>(),
                       e->d_logp.as<float>(), e->d_xlse.as<float>() + r0, e->d_xsum.as<double>() + r0, e->d_xtop.as<int>() + r0));
    else
      RVB_TRY(lse_gather_multi(e->stream, e->logits.as<float>(), rows, V, Vld, e->d_tgt_ptr.as<int>() + r0, e->d_tgt.as<int>(),
                               e->d_logp.as<float>()));
  }
  RVB_TRY(tap_keep(e, "logp", e->d_logp.p, (size_t)t.P, false));
  e->tap_live = false;
  logp->resize(t.P);
  RVB_HIP_CHECK(hipMemcpyAsync(logp->data(), e->d_logp.p, (size_t)t.P * 4, hipMemcpyDeviceToHost, e->stream));
  if (xent) {
    xent->lse.resize(R); xent->sum_x.resize(R); xent->top1.resize(R);
    RVB_HIP_CHECK(hipMemcpyAsync(xent->lse.data(), e->d_xlse.p, (size_t)R * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipMemcpyAsync(xent->sum_x.data(), e->d_xsum.p, (size_t)R * 8, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipMemcpyAsync(xent->top1.data(), e->d_xtop.p, (size_t)R * 4, hipMemcpyDeviceToHost, e->stream));
  }
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  return OK;
}

int rescore_impl(rvb_engine* e, double ctc_weight, double reverse_weight) {
  if ((int)e->nbest.size() != e->B || e->B <= 0) { set_error("rvb_attention_rescore before rvb_ctc_prefix_beam"); return E_STATE; }
  if (!e->dec_l.present) { set_error("model has no attention decoder"); return E_STATE; }
  RVB_TRY(wait_slices(e, -1));
  const bool use_r = reverse_weight > 0.0;
  if (use_r && !e->dec_r.present) { set_error("reverse_weight > 0 but model has no right-to-left decoder"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  const int B = e->B, T2 = e->T2, eos = e->cfg.eos_id, sos = e->cfg.sos_id;
  // every hypothesis of every chunk asks for len+1 log-probs ([sos] + tokens -> tokens + [eos]; add_sos_eos,
  // common.py:112-155, search.py:417-425)
  std::vector<HypRef> hyps;
  int P = 0;
  std::vector<int32_t> ckv(2 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    const PrefixResult& pr = e->nbest[b];
    ckv[b] = b * T2; ckv[B + b] = e->enc_lens[b];
    for (size_t i = 0; i < pr.nbest.size(); ++i) {
      const int len = (int)pr.nbest[i].size();
      if (len + 1 > e->pe_rows) { set_error("hypothesis longer than the positional table"); return E_UNSUPPORTED; }
      hyps.push_back({b, (int)i, len, P});
      P += len + 1;
    }
  }
  RVB_TRY(upload_i32(e, e->d_aux_i32, ckv.data(), ckv.size()));
  TrieBatch tl, tr;
  const auto th0 = std::chrono::steady_clock::now();
  if ((int)e->trie_l.size() == B) merge_tries(e->trie_l, &tl);      // built by the prefix-beam workers, chunk by chunk
  else build_trie_parallel(e, false, &tl);
  {
    auto& pe = e->prof["rescore_trie_host"];
    pe.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    pe.launches += 1;
  }
  std::vector<float> lslot, rslot;
  const auto td0 = std::chrono::steady_clock::now();
  RVB_TRY(decoder_forward(e, e->dec_l, tl, &lslot));
  {
    auto& pe = e->prof["rescore_decoder_wall"];
    pe.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td0).count();
    pe.launches += 1;
  }
  e->xattn_max_rows = tl.max_chunk_rows;
  e->rescore_rows = tl.R; e->rescore_pairs = tl.P;
  if (use_r) {   // reversed input and targets, asr_model.py:896-953, search.py:427-433
    build_trie_parallel(e, true, &tr);
    RVB_TRY(decoder_forward(e, e->dec_r, tr, &rslot));
    e->rescore_rows += tr.R; e->rescore_pairs += tr.P;
  }
  const auto ta0 = std::chrono::steady_clock::now();
  std::vector<float> logp(P), rlogp(use_r ? P : 0);
  for (int p = 0; p < P; ++p) { logp[p] = lslot[tl.pair_slot[p]]; if (use_r) rlogp[p] = rslot[tr.pair_slot[p]]; }

  // score accumulation exactly as search.py:413-441: fp32 running sums (0-dim float32 tensors), strict '>' so the first
  // maximum wins; the python-float exp() of the confidences is evaluated for the winning hypothesis only (the reference
  // computes them for every hypothesis and keeps the winner's)
  e->rescored.assign(B, RescoreResult());
  std::vector<float> att_score(hyps.size());        // decoder score before the CTC term (the confidence is derived from it)
  std::vector<int> best_hyp(B, -1);
  for (size_t hi = 0; hi < hyps.size(); ++hi) {
    const HypRef& hr = hyps[hi];
    const PrefixResult& pr = e->nbest[hr.chunk];
    RescoreResult& rr = e->rescored[hr.chunk];
    if (rr.logp.empty()) { rr.logp.resize(pr.nbest.size()); rr.rlogp.resize(pr.nbest.size()); rr.score = -INFINITY; }
    const float* lp = logp.data() + hr.row0;
    rr.logp[hr.idx].assign(lp, lp + hr.len + 1);
    float score = 0.f;
    for (int j = 0; j < hr.len; ++j) score += lp[j];
    score += lp[hr.len];
    if (use_r) {
      const float* rp = rlogp.data() + hr.row0;
      rr.rlogp[hr.idx].assign(rp, rp + hr.len + 1);
      float r_score = 0.f;
      for (int j = 0; j < hr.len; ++j) r_score += rp[hr.len - j - 1];
      r_score += rp[hr.len];
      // python: tensor(fp32) * float(1 - rw) + tensor(fp32) * float(rw)
      score = score * (float)(1.0 - reverse_weight) + r_score * (float)reverse_weight;
    }
    att_score[hi] = score;
    score += (float)(pr.scores[hr.idx] * ctc_weight);
    if (best_hyp[hr.chunk] < 0 || score > rr.score) { rr.score = score; rr.best = hr.idx; best_hyp[hr.chunk] = (int)hi; }
  }
  for (int b = 0; b < B; ++b) {
    RescoreResult& rr = e->rescored[b];
    if (best_hyp[b] < 0) { rr.best = 0; rr.score = -INFINITY; continue; }
    const HypRef& hr = hyps[best_hyp[b]];
    const float* lp = logp.data() + hr.row0;
    rr.confidence = std::exp((double)(att_score[best_hyp[b]] / (float)(hr.len + 1)));
    rr.tok_conf.resize(hr.len);
    for (int j = 0; j < hr.len; ++j) rr.tok_conf[j] = std::exp((double)lp[j]);
    if (use_r) {
      const float* rp = rlogp.data() + hr.row0;
      for (int j = 0; j < hr.len; ++j) rr.tok_conf[j] = (rr.tok_conf[j] + std::exp((double)rp[hr.len - j - 1])) / 2.0;
    }
  }
  {
    auto& pe = e->prof["rescore_scores_host"];
    pe.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta0).count();
    pe.launches += 1;
  }
  return OK;
}


// ------------------------------------------------------------------------------------ attention beam search
// `attention` mode (search.py:251-360): autoregressive beam search with the left decoder.  The reference's
// forward_one_step (decoder.py:191-234) recomputes the keys/values of the whole prefix at every step; here every
// decoder layer keeps a K/V cache per hypothesis ([R][L][d], reordered by the beam's parent index after each step),
// the memory K/V of each chunk is projected once, and one step is one decoder row per hypothesis.  The beam
// bookkeeping follows the reference line by line in float32.
int attention_decode_impl(rvb_engine* e, int N, float length_penalty) {
  const rvb_model_cfg& c = e->cfg;
  if (e->B <= 0) { set_error("rvb_attention_decode before rvb_encode"); return E_STATE; }
  if (!e->dec_l.present) { set_error("model has no attention decoder"); return E_STATE; }
  if (N < 1 || N > 64) { set_error("rvb_attention_decode: beam must be in 1..64"); return E_ARG; }
  RVB_TRY(wait_slices(e, -1));
  Decoder& D = e->dec_l;
  const int B = e->B, T2 = e->T2, d = c.d_model, heads = c.dec_heads, dk = d / heads, ff = c.dec_ffn_dim, V = c.vocab;
  const int eos = c.eos_id, sos = c.sos_id;
  const int R = B * N, L = T2, M = B * T2, NL = (int)D.layers.size();
  const size_t es = dt_size(e->dtype);
  if (L > e->pe_rows) { set_error("rvb_attention_decode: more steps than positional-table rows"); return E_UNSUPPORTED; }
  if (N > V) { set_error("rvb_attention_decode: beam larger than the vocabulary"); return E_ARG; }
  const int Vld = (V + 3) & ~3;

  e->kcache.resize(NL); e->vcache.resize(NL); e->kcache2.resize(NL); e->vcache2.resize(NL); e->memkv.resize(NL);
  const size_t cbytes = (size_t)R * L * d * es;
  for (int l = 0; l < NL; ++l) {
    RVB_TRY(e->kcache[l].ensure(cbytes)); RVB_TRY(e->vcache[l].ensure(cbytes));
    RVB_TRY(e->kcache2[l].ensure(cbytes)); RVB_TRY(e->vcache2[l].ensure(cbytes));
    RVB_TRY(e->memkv[l].ensure((size_t)M * 2 * d * es));
    RVB_TRY(run_gemm(e, e->enc_out.p, d, D.layers[l].src_kv, e->memkv[l].p, 2 * d, M, false));   // once per chunk, not per step
  }
  RVB_TRY(e->dx.ensure((size_t)R * d * 4));
  RVB_TRY(e->dxn.ensure((size_t)R * d * es));
  RVB_TRY(e->dy.ensure((size_t)R * d * es));
  RVB_TRY(e->dao.ensure((size_t)R * d * es));
  RVB_TRY(e->dq.ensure((size_t)R * d * es));
  RVB_TRY(e->dqkv.ensure((size_t)R * 3 * d * es));
  RVB_TRY(e->dh.ensure((size_t)R * ff * es));
  RVB_TRY(e->logits.ensure((size_t)std::min(R, LOGIT_SLAB) * Vld * 4));
  RVB_TRY(e->atopv.ensure((size_t)R * N * 4));
  RVB_TRY(e->atopi.ensure((size_t)R * N * 4));

  // sequence descriptors: self-attention = one query row per hypothesis against its cache rows [r*L, r*L + s];
  // cross-attention = the N hypotheses of a chunk form one query sequence against the chunk's valid frames
  std::vector<int32_t> q1(R), one(R, 1), kv0(R), kvl(R), cq(B), cn(B, N), ckv(2 * (size_t)B);
  for (int r = 0; r < R; ++r) { q1[r] = r; kv0[r] = r * L; }
  for (int b = 0; b < B; ++b) { cq[b] = b * N; ckv[b] = b * T2; ckv[B + b] = e->enc_lens[b]; }
  RVB_TRY(upload_i32(e, e->d_hq_start, q1.data(), R));
  RVB_TRY(upload_i32(e, e->d_hq_len, one.data(), R));
  RVB_TRY(upload_i32(e, e->d_seq_start, kv0.data(), R));
  RVB_TRY(upload_i32(e, e->d_hkv_start, cq.data(), B));
  RVB_TRY(upload_i32(e, e->d_hkv_len, cn.data(), B));
  RVB_TRY(upload_i32(e, e->d_aux_i32, ckv.data(), ckv.size()));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));

  std::vector<std::vector<int>> hyps(R, std::vector<int>(1, sos));
  std::vector<float> scores(R, -INFINITY);
  for (int b = 0; b < B; ++b) scores[(size_t)b * N] = 0.f;            // search.py:289-292
  std::vector<char> end_flag(R, 0);
  // (a chunk without a single valid encoder frame is NOT special-cased: the reference decodes it against a fully masked
  // memory -- attention output zero, attention.py:112-114 -- and emits whatever the decoder's prior produces; the golden
  // case tiny_bn has such a 5-frame tail chunk)
  std::vector<int32_t> tok(R), pos(R), parent(R);
  std::vector<float> topv((size_t)R * N);
  std::vector<int32_t> topi((size_t)R * N);
  float* x = e->dx.as<float>();

  for (int s = 0; s < L; ++s) {                                        // i = s + 1 in search.py:296
    int n_end = 0;
    for (int r = 0; r < R; ++r) n_end += end_flag[r];
    if (n_end == R) break;
    for (int r = 0; r < R; ++r) { tok[r] = hyps[r].back(); pos[r] = s; kvl[r] = s + 1; }
    RVB_TRY(upload_i32(e, e->d_tok, tok.data(), R));
    RVB_TRY(upload_i32(e, e->d_pos, pos.data(), R));
    RVB_TRY(upload_i32(e, e->d_seq_len, kvl.data(), R));
    {
      Scope sc(e, "embed");
      RVB_TRY(embed_tokens(e->stream, D.embed.as<float>(), e->pe_f32.as<float>(), e->d_tok.as<int>(), e->d_pos.as<int>(), x, R, d,
                           std::sqrt((float)d)));
    }
    for (int l = 0; l < NL; ++l) {
      DecLayer& Ly = D.layers[l];
      RVB_TRY(run_norm(e, x, Ly.n1, e->dxn.p, false, R, d));
      RVB_TRY(run_gemm(e, e->dxn.p, d, Ly.self_qkv, e->dqkv.p, 3 * d, R, false));
      RVB_HIP_CHECK(hipMemcpy2DAsync((char*)e->kcache[l].p + (size_t)s * d * es, (size_t)L * d * es, (const char*)e->dqkv.p + (size_t)d * es,
                                     (size_t)3 * d * es, (size_t)d * es, R, hipMemcpyDeviceToDevice, e->stream));
      RVB_HIP_CHECK(hipMemcpy2DAsync((char*)e->vcache[l].p + (size_t)s * d * es, (size_t)L * d * es, (const char*)e->dqkv.p + (size_t)2 * d * es,
                                     (size_t)3 * d * es, (size_t)d * es, R, hipMemcpyDeviceToDevice, e->stream));
      AttnArgs a;
      memset(&a, 0, sizeof(a));
      a.q = e->dqkv.p; a.k = e->kcache[l].p; a.v = e->vcache[l].p;
      a.q_stride = 3 * d; a.k_stride = a.v_stride = d; a.o_stride = d; a.out = e->dao.p;
      a.q_start = e->d_hq_start.as<int>(); a.q_len = e->d_hq_len.as<int>();
      a.kv_start = e->d_seq_start.as<int>(); a.kv_len = e->d_seq_len.as<int>();
      a.nseq = R; a.heads = heads; a.dk = dk; a.max_q = 1; a.causal = 0; a.sqrt_dk = std::sqrt((float)dk);
      { Scope sc(e, "attention"); RVB_TRY(attention(e->stream, e->dtype, with_lab(a))); }
      RVB_TRY(run_gemm(e, e->dao.p, d, Ly.self_out, x, d, R, true, 1.f, ACT_NONE, x, d));
      RVB_TRY(run_norm(e, x, Ly.n2, e->dxn.p, false, R, d));
      RVB_TRY(run_gemm(e, e->dxn.p, d, Ly.src_q, e->dq.p, d, R, false));
      a.q = e->dq.p; a.k = e->memkv[l].p; a.v = (const char*)e->memkv[l].p + (size_t)d * es;
      a.q_stride = d; a.k_stride = a.v_stride = 2 * d;
      a.q_start = e->d_hkv_start.as<int>(); a.q_len = e->d_hkv_len.as<int>();
      a.kv_start = e->d_aux_i32.as<int>(); a.kv_len = e->d_aux_i32.as<int>() + B;
      a.nseq = B; a.max_q = N;
      { Scope sc(e, "attention"); RVB_TRY(attention(e->stream, e->dtype, with_lab(a))); }
      RVB_TRY(run_gemm(e, e->dao.p, d, Ly.src_out, x, d, R, true, 1.f, ACT_NONE, x, d));
      RVB_TRY(run_norm(e, x, Ly.n3, e->dxn.p, false, R, d));
      const void* ffin = e->dxn.p;
      if (Ly.is_lsl) { RVB_TRY(run_gemm(e, e->dxn.p, d, Ly.lsl, e->dy.p, d, R, false)); ffin = e->dy.p; }
      RVB_TRY(run_gemm(e, ffin, d, Ly.ff1, e->dh.p, ff, R, false, 1.f, ACT_RELU));
      RVB_TRY(run_gemm(e, e->dh.p, ff, Ly.ff2, x, d, R, true, 1.f, ACT_NONE, x, d));
    }
    RVB_TRY(run_norm(e, x, D.after, e->dxn.p, false, R, d));
    for (int r0 = 0; r0 < R; r0 += LOGIT_SLAB) {
      const int rows = std::min(LOGIT_SLAB, R - r0);
      RVB_TRY(run_gemm(e, (const char*)e->dxn.p + (size_t)r0 * d * es, d, D.out, e->logits.p, Vld, rows, true));
      Scope sc(e, "ctc_topk");
      RVB_TRY(logsoftmax_topk(e->stream, e->logits.as<float>(), rows, V, Vld, N, 0.f, 0, e->atopv.as<float>() + (size_t)r0 * N,
                              e->atopi.as<int>() + (size_t)r0 * N, nullptr));
    }
    RVB_HIP_CHECK(hipMemcpyAsync(topv.data(), e->atopv.p, (size_t)R * N * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipMemcpyAsync(topi.data(), e->atopi.p, (size_t)R * N * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));

    // ---- beam update, search.py:300-345 ----
    bool moved = false;
    std::vector<std::vector<int>> nh(R);
    std::vector<float> ns(R);
    std::vector<std::pair<float, int>> cand((size_t)N * N);
    for (int b = 0; b < B; ++b) {
      for (int n = 0; n < N; ++n) {
        const int r = b * N + n;
        for (int k = 0; k < N; ++k) {
          float lp = topv[(size_t)r * N + k];
          if (end_flag[r]) lp = k == 0 ? 0.f : -INFINITY;             // mask_finished_scores
          cand[(size_t)n * N + k] = {scores[r] + lp, n * N + k};
        }
      }
      // torch.topk: descending; equal values keep the lower index first
      std::stable_sort(cand.begin(), cand.end(), [](const std::pair<float, int>& a, const std::pair<float, int>& b2) { return a.first > b2.first; });
      for (int n = 0; n < N; ++n) {
        const int off = cand[n].second, pn = off / N, pk = off % N;
        const int pr = b * N + pn, r = b * N + n;
        const int pred = end_flag[pr] ? eos : topi[(size_t)pr * N + pk];   // mask_finished_preds
        nh[r] = hyps[pr];
        nh[r].push_back(pred);
        ns[r] = cand[n].first;
        parent[r] = pr;
        moved |= pr != r;
      }
    }
    hyps.swap(nh);
    scores.swap(ns);
    for (int r = 0; r < R; ++r) end_flag[r] = hyps[r].back() == eos;
    if (moved && s + 1 < L) {
      RVB_TRY(upload_i32(e, e->d_tgt, parent.data(), R));
      for (int l = 0; l < NL; ++l) {
        RVB_TRY(gather_cache(e->stream, e->kcache[l].p, e->kcache2[l].p, e->d_tgt.as<int>(), R, L, s + 1, (int)(d * es)));
        RVB_TRY(gather_cache(e->stream, e->vcache[l].p, e->vcache2[l].p, e->d_tgt.as<int>(), R, L, s + 1, (int)(d * es)));
        std::swap(e->kcache[l], e->kcache2[l]);
        std::swap(e->vcache[l], e->vcache2[l]);
      }
    }
  }
  // ---- best of the beam, search.py:347-360 (float32 like the tensors there) ----
  e->attn_tokens.assign(B, {});
  e->attn_scores.assign(B, 0.f);
  for (int b = 0; b < B; ++b) {
    float best = -INFINITY;
    int bi = 0;
    for (int n = 0; n < N; ++n) {
      const std::vector<int>& h = hyps[(size_t)b * N + n];
      int len = 0;
      for (int t : h) len += t != eos;
      const float sc = scores[(size_t)b * N + n] / std::pow((float)len, length_penalty);
      if (n == 0 || sc > best) { best = sc; bi = n; }
    }
    const std::vector<int>& h = hyps[(size_t)b * N + bi];
    for (size_t j = 1; j < h.size(); ++j) if (h[j] != eos) e->attn_tokens[b].push_back(h[j]);
    e->attn_scores[b] = best;
  }
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  return OK;
}


// ------------------------------------------------------------------------------------ joint_decoding
// `joint_decoding` (transformer/search.py:450-496 -> espnet/beam_search_timesync.py:86-508): time-synchronous joint CTC /
// attention beam search.  The reference runs one BeamSearchTimeSync per chunk and, inside it, the attention decoder on ONE
// new prefix at a time, re-feeding the whole prefix with the cached layer outputs of its parent (cached_score :185-224).
// Here every chunk of the batch advances in lockstep, one encoder frame per iteration:
//   * the CTC half of the frame and the joint scoring run on the host, per chunk (search.cpp JointSearch: the reference's
//     float64 arithmetic and dict semantics on a prefix trie);
//   * the prefixes whose decoder output is needed for the first time -- of ALL chunks -- form one batched decoder step:
//     one row per prefix (its last token), self-attention over the key / value rows of its ancestors (kept per decoder
//     layer for every decoded prefix, addressed through AttnArgs::kv_index), cross-attention against the chunk's memory
//     keys / values (projected once), output layer, log-softmax row kept on the device;
//   * the (prefix, next token) log-probs the joint scores need are gathered from those rows and copied back: a few
//     floats per chunk and frame.
// The memory is the chunk's valid frames, as the class's own `reset` expects ((1, len, d); the reference's call passes a
// 2-D tensor and fails there -- DESIGN.md, oracle/gen_golden_joint.py).
static int grow_rows(rvb_engine* e, DevBuf& b, size_t row_bytes, int64_t have, int64_t need) {
  if ((size_t)need * row_bytes <= b.bytes) return OK;
  DevBuf nb;
  const int64_t cap = std::max<int64_t>(need, (int64_t)(b.bytes / row_bytes) * 2);
  RVB_TRY(nb.ensure((size_t)cap * row_bytes));
  if (have > 0) RVB_HIP_CHECK(hipMemcpyAsync(nb.p, b.p, (size_t)have * row_bytes, hipMemcpyDeviceToDevice, e->stream));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  b.release();
  b = nb;
  nb.p = nullptr; nb.bytes = 0;
  return OK;
}

// a few persistent host threads for the per-chunk halves of a joint_decoding frame (512 frames per batch: starting threads
// per frame would cost more than the work)
namespace {
class FramePool {
 public:
  explicit FramePool(unsigned n) {
    for (unsigned i = 1; i < n; ++i) th_.emplace_back([this, i] { loop((int)i); });
  }
  ~FramePool() {
    { std::lock_guard<std::mutex> g(m_); stop_ = true; ++gen_; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // fn(i) for i in [0, n); item i always runs on participant i mod P (the caller is participant 0), so that a chunk's
  // search state is touched -- and its vectors are grown and freed -- by one thread only
  template <typename F> void run(int n, F&& fn) {
    if (th_.empty() || n < 8) { for (int i = 0; i < n; ++i) fn(i); return; }
    job_ = [&fn](int i) { fn(i); };
    { std::lock_guard<std::mutex> g(m_); n_ = n; busy_ = (int)th_.size(); ++gen_; }
    cv_.notify_all();
    work(0);
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this] { return busy_ == 0; });
  }

 private:
  void work(int id) { const int P = (int)th_.size() + 1; for (int i = id; i < n_; i += P) job_(i); }
  void loop(int id) {
    int seen = 0;
    for (;;) {
      { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return gen_ != seen; }); seen = gen_; if (stop_) return; }
      work(id);
      { std::lock_guard<std::mutex> g(m_); if (--busy_ == 0) done_.notify_one(); }
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  std::function<void(int)> job_;
  int n_ = 0, busy_ = 0, gen_ = 0;
  bool stop_ = false;
};
}  // namespace

int joint_decode_impl(rvb_engine* e, int beam, double ctc_weight, double pre_beam_ratio, double length_bonus) {
  const rvb_model_cfg& c = e->cfg;
  if (e->B <= 0) { set_error("rvb_joint_decode before rvb_encode"); return E_STATE; }
  if (!e->dec_l.present) { set_error("model has no attention decoder"); return E_STATE; }
  const int pre_beam = (int)(pre_beam_ratio * beam);
  if (beam < 1 || pre_beam < 1) { set_error("rvb_joint_decode: beam and pre_beam_ratio * beam must be >= 1"); return E_ARG; }
  if (pre_beam > e->beam) {
    set_error("rvb_joint_decode: rvb_encode kept the top " + std::to_string(e->beam) + " CTC log-probs per frame, the pre-beam needs " +
              std::to_string(pre_beam));
    return E_ARG;
  }
  RVB_TRY(wait_slices(e, -1));
  Decoder& D = e->dec_l;
  const int B = e->B, T2 = e->T2, d = c.d_model, heads = c.dec_heads, dk = d / heads, ff = c.dec_ffn_dim, V = c.vocab;
  const int M = B * T2, NL = (int)D.layers.size(), K = e->beam;
  const size_t es = dt_size(e->dtype);
  const int Vld = (V + 3) & ~3;
  if (T2 + 1 > e->pe_rows) { set_error("rvb_joint_decode: more positions than positional-table rows"); return E_UNSUPPORTED; }

  // ---- per-frame log-prob of token 0 (the reference's blank-skip test reads p_ctc[0]) and of the blank
  std::vector<float> p0(M), pbl(M);
  {
    RVB_TRY(e->logits.ensure((size_t)LOGIT_SLAB * Vld * 4));
    RVB_TRY(e->d_tgt.ensure((size_t)LOGIT_SLAB * 4));
    RVB_TRY(e->d_logp.ensure((size_t)LOGIT_SLAB * 4));
    std::vector<int32_t> tgt(LOGIT_SLAB);
    for (int pass = 0; pass < (c.blank_id == 0 ? 1 : 2); ++pass) {
      std::fill(tgt.begin(), tgt.end(), pass == 0 ? 0 : c.blank_id);
      RVB_TRY(upload_i32(e, e->d_tgt, tgt.data(), LOGIT_SLAB));
      std::vector<float>& dst = pass == 0 ? p0 : pbl;
      for (int r0 = 0; r0 < M; r0 += LOGIT_SLAB) {
        const int rows = std::min(LOGIT_SLAB, M - r0);
        RVB_TRY(run_gemm(e, (const char*)e->enc_out.p + (size_t)r0 * d * es, d, e->ctc, e->logits.p, Vld, rows, true));
        // with a blank penalty the reference's CTC log-probs are the log-softmax of the PENALISED logits (ctc_logprobs,
        // asr_model.py:318-329; search.py:466): the same rows the top-k kernel produced for this batch
        RVB_TRY(lse_gather(e->stream, e->logits.as<float>(), rows, V, Vld, e->d_tgt.as<int>(), e->d_logp.as<float>(), e->last_blank_penalty,
                           c.blank_id));
        RVB_HIP_CHECK(hipMemcpyAsync(dst.data() + r0, e->d_logp.p, (size_t)rows * 4, hipMemcpyDeviceToHost, e->stream));
        RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
      }
    }
    if (c.blank_id == 0) pbl = p0;
  }

  // ---- memory keys / values of every chunk, once per decoder layer
  e->memkv.resize(NL); e->jkv.resize(NL);
  for (int l = 0; l < NL; ++l) {
    RVB_TRY(e->memkv[l].ensure((size_t)M * 2 * d * es));
    RVB_TRY(run_gemm(e, e->enc_out.p, d, D.layers[l].src_kv, e->memkv[l].p, 2 * d, M, false));
  }
  const int Rmax = B * std::max(beam, 1);
  RVB_TRY(e->dx.ensure((size_t)Rmax * d * 4));
  RVB_TRY(e->dxn.ensure((size_t)Rmax * d * es));
  RVB_TRY(e->dy.ensure((size_t)Rmax * d * es));
  RVB_TRY(e->dao.ensure((size_t)Rmax * d * es));
  RVB_TRY(e->dq.ensure((size_t)Rmax * d * es));
  RVB_TRY(e->dqkv.ensure((size_t)Rmax * 3 * d * es));
  RVB_TRY(e->dh.ensure((size_t)Rmax * ff * es));
  RVB_TRY(e->logits.ensure((size_t)std::max(Rmax, LOGIT_SLAB) * Vld * 4));
  RVB_TRY(e->atopv.ensure((size_t)Rmax * 4));
  RVB_TRY(e->atopi.ensure((size_t)Rmax * 4));

  JointParams jp;
  jp.beam = beam; jp.pre_beam = pre_beam; jp.blank = c.blank_id; jp.sos = c.sos_id;
  jp.w_ctc = ctc_weight; jp.w_dec = 1.0 - ctc_weight; jp.bonus = length_bonus; jp.log_thr = 0.0;
  std::vector<JointSearch> js;
  js.reserve(B);
  for (int b = 0; b < B; ++b) js.emplace_back(jp);
  int64_t next_row = 0;
  e->joint_rows = 0; e->joint_steps = 0;
  float* x = e->dx.as<float>();

  // one batched decoder step for the prefixes (chunk, node) in `req` (grouped by chunk, in order)
  struct Req { int chunk, node; };
  std::vector<int32_t> tok, pos, q1, one, pstart, plen, path, xq0, xqn, xkv;
  auto step = [&](const std::vector<Req>& req) -> int {
    const int R = (int)req.size();
    if (R == 0) return OK;
    if (R > Rmax) { set_error("rvb_joint_decode: more new prefixes in one frame than beam x chunks"); return E_STATE; }
    const int64_t row0 = next_row;
    for (int l = 0; l < NL; ++l) RVB_TRY(grow_rows(e, e->jkv[l], (size_t)2 * d * es, row0, row0 + R));
    RVB_TRY(grow_rows(e, e->jlogp, (size_t)V * 4, row0, row0 + R));
    tok.resize(R); pos.resize(R); q1.resize(R); one.assign(R, 1); pstart.resize(R); plen.resize(R);
    path.clear(); xq0.clear(); xqn.clear(); xkv.clear();
    std::vector<int32_t> xk0, xkn;
    int max_xq = 0;
    for (int r = 0; r < R; ++r) {
      JointSearch& J = js[req[r].chunk];
      const int node = req[r].node;
      J.set_tag(node, (int)(row0 + r));
      const int len = J.length(node);
      tok[r] = J.token(node); pos[r] = len - 1; q1[r] = r;
      pstart[r] = (int)path.size(); plen[r] = len;
      const size_t at = path.size();
      path.resize(at + len);
      for (int n = node, i = len - 1; n >= 0; n = J.parent(n), --i) path[at + i] = J.tag(n);   // ancestors are decoded
      if (r == 0 || req[r].chunk != req[r - 1].chunk) { xq0.push_back(r); xqn.push_back(0); xk0.push_back(req[r].chunk * T2); xkn.push_back(e->enc_lens[req[r].chunk]); }
      max_xq = std::max(max_xq, ++xqn.back());
    }
    const int nx = (int)xq0.size();
    xkv = xk0; xkv.insert(xkv.end(), xkn.begin(), xkn.end());
    RVB_TRY(upload_i32(e, e->d_tok, tok.data(), R));
    RVB_TRY(upload_i32(e, e->d_pos, pos.data(), R));
    RVB_TRY(upload_i32(e, e->d_hq_start, q1.data(), R));
    RVB_TRY(upload_i32(e, e->d_hq_len, one.data(), R));
    RVB_TRY(upload_i32(e, e->d_hpath_start, pstart.data(), R));
    RVB_TRY(upload_i32(e, e->d_hpath_len, plen.data(), R));
    RVB_TRY(upload_i32(e, e->d_path, path.data(), path.size()));
    RVB_TRY(upload_i32(e, e->d_hkv_start, xq0.data(), nx));
    RVB_TRY(upload_i32(e, e->d_hkv_len, xqn.data(), nx));
    RVB_TRY(upload_i32(e, e->d_aux_i32, xkv.data(), xkv.size()));
    {
      Scope sc(e, "embed");
      RVB_TRY(embed_tokens(e->stream, D.embed.as<float>(), e->pe_f32.as<float>(), e->d_tok.as<int>(), e->d_pos.as<int>(), x, R, d,
                           std::sqrt((float)d)));
    }
    for (int l = 0; l < NL; ++l) {
      DecLayer& Ly = D.layers[l];
      RVB_TRY(run_norm(e, x, Ly.n1, e->dxn.p, false, R, d));
      RVB_TRY(run_gemm(e, e->dxn.p, d, Ly.self_qkv, e->dqkv.p, 3 * d, R, false));
      // the new prefixes' key | value rows join the per-layer store (k and v are adjacent in the fused projection)
      RVB_HIP_CHECK(hipMemcpy2DAsync((char*)e->jkv[l].p + (size_t)row0 * 2 * d * es, (size_t)2 * d * es, (const char*)e->dqkv.p + (size_t)d * es,
                                     (size_t)3 * d * es, (size_t)2 * d * es, R, hipMemcpyDeviceToDevice, e->stream));
      AttnArgs a;
      memset(&a, 0, sizeof(a));
      a.q = e->dqkv.p; a.k = e->jkv[l].p; a.v = (const char*)e->jkv[l].p + (size_t)d * es;
      a.q_stride = 3 * d; a.k_stride = a.v_stride = 2 * d; a.o_stride = d; a.out = e->dao.p;
      a.q_start = e->d_hq_start.as<int>(); a.q_len = e->d_hq_len.as<int>();
      a.kv_start = e->d_hpath_start.as<int>(); a.kv_len = e->d_hpath_len.as<int>(); a.kv_index = e->d_path.as<int>();
      a.nseq = R; a.heads = heads; a.dk = dk; a.max_q = 1; a.causal = 0; a.sqrt_dk = std::sqrt((float)dk);
      { Scope sc(e, "attention"); RVB_TRY(attention(e->stream, e->dtype, with_lab(a))); }
      RVB_TRY(run_gemm(e, e->dao.p, d, Ly.self_out, x, d, R, true, 1.f, ACT_NONE, x, d));
      RVB_TRY(run_norm(e, x, Ly.n2, e->dxn.p, false, R, d));
      RVB_TRY(run_gemm(e, e->dxn.p, d, Ly.src_q, e->dq.p, d, R, false));
      memset(&a, 0, sizeof(a));
      a.q = e->dq.p; a.k = e->memkv[l].p; a.v = (const char*)e->memkv[l].p + (size_t)d * es;
      a.q_stride = d; a.k_stride = a.v_stride = 2 * d; a.o_stride = d; a.out = e->dao.p;
      a.q_start = e->d_hkv_start.as<int>(); a.q_len = e->d_hkv_len.as<int>();
      a.kv_start = e->d_aux_i32.as<int>(); a.kv_len = e->d_aux_i32.as<int>() + nx;
      a.nseq = nx; a.heads = heads; a.dk = dk; a.max_q = max_xq; a.causal = 0; a.sqrt_dk = std::sqrt((float)dk);
      { Scope sc(e, "attention"); RVB_TRY(attention(e->stream, e->dtype, with_lab(a))); }
      RVB_TRY(run_gemm(e, e->dao.p, d, Ly.src_out, x, d, R, true, 1.f, ACT_NONE, x, d));
      RVB_TRY(run_norm(e, x, Ly.n3, e->dxn.p, false, R, d));
      const void* ffin = e->dxn.p;
      if (Ly.is_lsl) { RVB_TRY(run_gemm(e, e->dxn.p, d, Ly.lsl, e->dy.p, d, R, false)); ffin = e->dy.p; }
      RVB_TRY(run_gemm(e, ffin, d, Ly.ff1, e->dh.p, ff, R, false, 1.f, ACT_RELU));
      RVB_TRY(run_gemm(e, e->dh.p, ff, Ly.ff2, x, d, R, true, 1.f, ACT_NONE, x, d));
    }
    RVB_TRY(run_norm(e, x, D.after, e->dxn.p, false, R, d));
    RVB_TRY(run_gemm(e, e->dxn.p, d, D.out, e->logits.p, Vld, R, true));
    {
      Scope sc(e, "ctc_topk");
      RVB_TRY(logsoftmax_topk(e->stream, e->logits.as<float>(), R, V, Vld, 1, 0.f, 0, e->atopv.as<float>(), e->atopi.as<int>(),
                              e->jlogp.as<float>() + (size_t)row0 * V));
    }
    next_row += R;
    e->joint_rows += R; e->joint_steps += 1;
    return OK;
  };

  // reset(): the decoder on <sos> for every chunk
  std::vector<Req> req;
  for (int b = 0; b < B; ++b) req.push_back({b, 0});
  RVB_TRY(step(req));

  int Tmax = 0;
  for (int b = 0; b < B; ++b) Tmax = std::max(Tmax, e->enc_lens[b]);
  std::vector<int> npairs(B), ran(B);
  std::vector<std::vector<int>> cdec(B), cpn(B), cpt(B);
  std::vector<size_t> pair_at(B + 1);
  FramePool pool(std::min<unsigned>(search_threads(), 16u));
  std::vector<int32_t> prow, ptok;
  std::vector<float> vals;
  for (int t = 0; t < Tmax; ++t) {
    req.clear(); prow.clear(); ptok.clear();
    pool.run(B, [&](int b) {                     // CTC half of the frame, chunk by chunk on the host threads
      ran[b] = 0; cdec[b].clear(); cpn[b].clear(); cpt[b].clear();
      if (t >= e->enc_lens[b]) return;
      const size_t f = (size_t)b * T2 + t;
      ran[b] = js[b].begin_frame(t, e->h_topv + f * K, e->h_topi + f * K, K, p0[f], pbl[f], &cdec[b], &cpn[b], &cpt[b]) ? 1 : 0;
    });
    for (int b = 0; b < B; ++b) {
      npairs[b] = 0;
      if (!ran[b]) continue;
      for (int n : cdec[b]) req.push_back({b, n});
      npairs[b] = (int)cpn[b].size();
      for (size_t i = 0; i < cpn[b].size(); ++i) { prow.push_back(-1 - cpn[b][i]); ptok.push_back(cpt[b][i]); }      // rows resolved after the step
    }
    RVB_TRY(step(req));
    {   // pair rows: the node's tag is known now
      size_t at = 0;
      for (int b = 0; b < B; ++b)
        for (int i = 0; i < npairs[b]; ++i, ++at) prow[at] = js[b].tag(-1 - prow[at]);
    }
    const int NP = (int)prow.size();
    vals.resize(std::max(NP, 1));
    if (NP > 0) {
      RVB_TRY(e->jpair_row.ensure((size_t)NP * 4)); RVB_TRY(e->jpair_tok.ensure((size_t)NP * 4)); RVB_TRY(e->jpair_out.ensure((size_t)NP * 4));
      RVB_TRY(upload_i32(e, e->jpair_row, prow.data(), NP));
      RVB_TRY(upload_i32(e, e->jpair_tok, ptok.data(), NP));
      RVB_TRY(gather_pairs(e->stream, e->jlogp.as<float>(), (size_t)V, e->jpair_row.as<int>(), e->jpair_tok.as<int>(), NP, e->jpair_out.as<float>()));
      RVB_HIP_CHECK(hipMemcpyAsync(vals.data(), e->jpair_out.p, (size_t)NP * 4, hipMemcpyDeviceToHost, e->stream));
      RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    pair_at[0] = 0;
    for (int b = 0; b < B; ++b) pair_at[b + 1] = pair_at[b] + (size_t)npairs[b];
    pool.run(B, [&](int b) { if (ran[b]) js[b].finish_frame(vals.data() + pair_at[b]); });
  }
  e->joint.assign(B, JointResult());
  for (int b = 0; b < B; ++b) js[b].result(&e->joint[b]);
  for (int b = 0; b < B; ++b)
    if (js[b].ties_cut() && K < V) {
      set_error("rvb_joint_decode: a frame of chunk " + std::to_string(b) + " has more than " + std::to_string(K - pre_beam) +
                " log-probs that tie exactly with the pre-beam threshold; keep more per frame (rvb_encode's beam argument, up to 64)");
      return E_UNSUPPORTED;
    }
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
  return OK;
}

}  // namespace rvb

using namespace rvb;

extern "C" {

// Teacher-forced decoder pass over GIVEN sequences (ASRModel._calc_att_loss, asr_model.py:248-286): the rescoring decoder on a trie
// built from the caller's sequences, row_xent in place of lse_gather_multi, and the label-smoothed KL of label_smoothing_loss.py:68-96
// composed per position in fp64 from its closed form: with u = smoothing / (V - 1), c = 1 - smoothing and sum_v log p(v) =
// sum_x - V lse,   kl = c ln c + (V - 1) u ln u - c logp_t - u (sum_x - V lse - logp_t)      (0 ln 0 = 0)
int rvb_attention_score(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* chunk_of,
                        double reverse_weight, double lsm_weight, double* loss_l, double* loss_r, int32_t* n_correct,
                        int32_t* n_positions, float* logp_l, float* logp_r, int32_t* top1_l) {
  const std::string w("rvb_attention_score");
  if (!e) { set_error(w + ": null engine"); return E_ARG; }
  if (!tokens || !tok_lens || !chunk_of || !loss_l || n_seq <= 0) { set_error(w + ": null argument or n_seq <= 0"); return E_ARG; }
  if (e->B <= 0) { set_error(w + " before rvb_encode"); return E_STATE; }
  if (!e->dec_l.present) { set_error(w + ": model has no attention decoder"); return E_STATE; }
  const bool use_r = reverse_weight > 0.0;
  if (use_r && !e->dec_r.present) { set_error(w + ": reverse_weight > 0 but model has no right-to-left decoder"); return E_STATE; }
  const int B = e->B, T2 = e->T2, V = e->cfg.vocab, eos = e->cfg.eos_id, sos = e->cfg.sos_id;
  if (!(lsm_weight >= 0.0 && lsm_weight < 1.0) || !(reverse_weight >= 0.0 && reverse_weight <= 1.0) || V < 2) {
    set_error(w + ": need 0 <= lsm_weight < 1, 0 <= reverse_weight <= 1 and a vocabulary of at least 2"); return E_ARG;
  }
  std::vector<int64_t> tok_off(n_seq), pos_off(n_seq);
  int64_t nt = 0, np = 0;
  for (int i = 0; i < n_seq; ++i) {
    const int L = tok_lens[i];
    const std::string at = w + ": sequence " + std::to_string(i) + ": ";
    if (L <= 0) { set_error(at + "empty transcript (L = 0): nothing to score"); return E_ARG; }
    if (chunk_of[i] < 0 || chunk_of[i] >= B) {
      set_error(at + "chunk " + std::to_string(chunk_of[i]) + " outside the encoded batch of " + std::to_string(B) + " chunks"); return E_ARG;
    }
    for (int k = 0; k < L; ++k) {
      const int y = tokens[nt + k];
      if (y < 0 || y >= V) { set_error(at + "token id " + std::to_string(y) + " outside [0, " + std::to_string(V) + ")"); return E_ARG; }
    }
    if (L + 1 > e->pe_rows) {
      set_error(at + std::to_string(L) + " tokens + <eos> are longer than the positional table of " + std::to_string(e->pe_rows) + " rows");
      return E_UNSUPPORTED;
    }
    tok_off[i] = nt; pos_off[i] = np;
    nt += L; np += L + 1;
  }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(wait_slices(e, -1));
  // the sequences in chunk order (build_trie_range walks chunk by chunk); candidates of one chunk share the rows of common prefixes
  std::vector<int> order(n_seq);
  for (int i = 0; i < n_seq; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return chunk_of[a] < chunk_of[b]; });
  std::vector<HypRef> hyps(n_seq);
  int P = 0;
  for (int k = 0; k < n_seq; ++k) { const int i = order[k]; hyps[k] = {chunk_of[i], i, tok_lens[i], P}; P += tok_lens[i] + 1; }
  std::vector<int32_t> ckv(2 * (size_t)B);
  for (int b = 0; b < B; ++b) { ckv[b] = b * T2; ckv[B + b] = e->enc_lens[b]; }
  RVB_TRY(upload_i32(e, e->d_aux_i32, ckv.data(), ckv.size()));
  const double c = 1.0 - lsm_weight, u = lsm_weight / (double)(V - 1);
  const double k0 = (c > 0.0 ? c * std::log(c) : 0.0) + (u > 0.0 ? (double)(V - 1) * u * std::log(u) : 0.0);
  for (int side = 0; side < (use_r ? 2 : 1); ++side) {
    TrieBatch t;
    if (side == 0)
      build_trie_range(hyps.data(), hyps.data() + n_seq, 0, B, sos, eos,
                       [&](const HypRef& h, int j) { return tokens[tok_off[h.idx] + j]; }, &t);
    else       // reverse_pad_list + add_sos_eos: the reversed tokens, then <eos>
      build_trie_range(hyps.data(), hyps.data() + n_seq, 0, B, sos, eos,
                       [&](const HypRef& h, int j) { return tokens[tok_off[h.idx] + h.len - 1 - j]; }, &t);
    std::vector<float> slot;
    XentRows xr;
    RVB_TRY(decoder_forward(e, side == 0 ? e->dec_l : e->dec_r, t, &slot, &xr));
    for (int k = 0; k < n_seq; ++k) {
      const HypRef& h = hyps[k];
      double loss = 0.0;
      int correct = 0;
      for (int j = 0; j <= h.len; ++j) {
        const int sl = t.pair_slot[h.row0 + j], row = t.path[t.hkv_start[k] + j];
        const double lp = (double)slot[sl];
        loss += k0 - c * lp - u * (xr.sum_x[row] - (double)V * (double)xr.lse[row] - lp);
        correct += xr.top1[row] == t.tgt[sl];
        if (side == 0) {
          if (logp_l) logp_l[pos_off[h.idx] + j] = slot[sl];
          if (top1_l) top1_l[pos_off[h.idx] + j] = xr.top1[row];
        } else if (logp_r) {
          logp_r[pos_off[h.idx] + j] = slot[sl];
        }
      }
      if (side == 0) {
        loss_l[h.idx] = loss;
        if (n_correct) n_correct[h.idx] = correct;
        if (n_positions) n_positions[h.idx] = h.len + 1;
      } else if (loss_r) {
        loss_r[h.idx] = loss;
      }
    }
  }
  if (!use_r && loss_r) for (int i = 0; i < n_seq; ++i) loss_r[i] = 0.0;
  return OK;
}

int rvb_set_decoder_tap(rvb_engine* e, int side, int position) {
  const std::string w("rvb_set_decoder_tap");
  if (!e) { set_error(w + ": null engine"); return E_ARG; }
  if (!e->finalized) { set_error(w + " before rvb_finalize"); return E_STATE; }
  if (side != 0 && side != 1) { set_error(w + ": side must be 0 (left decoder) or 1 (right decoder)"); return E_ARG; }
  const Decoder& D = side ? e->dec_r : e->dec_l;
  if (position >= 0 && !D.present) { set_error(w + ": the model has no such decoder"); return E_STATE; }
  if (position < -1 || position > (int)D.layers.size()) {
    set_error(w + ": position must be -1 (off), 0 .. layers - 1, or layers (the head)"); return E_ARG;
  }
  if (position >= 0 && e->fp8) { set_error(w + ": not available on an fp8 engine"); return E_UNSUPPORTED; }
  if (position != e->dtap_pos || side != e->dtap_side) {       // another position, or off: what the taps held is given back
    RVB_HIP_CHECK(hipSetDevice(e->device));
    RVB_TRY(wait_slices(e, -1));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));
    for (auto& t : e->dtaps) t.second.buf.release();
    e->dtaps.clear(); e->dtap_forms.clear(); e->dtap_trie.clear(); e->dtap_rows = 0;
  }
  e->dtap_side = side; e->dtap_pos = position;
  return OK;
}
int rvb_get_decoder_tap(rvb_engine* e, const char* name, float* out, int64_t capacity) {
  const std::string w("rvb_get_decoder_tap: ");
  if (!e || !name || !out) { set_error(w + "null argument"); return E_ARG; }
  const bool forms = !strcmp(name, "forms"), dims = !strcmp(name, "trie_dims"), trie = dims || !strcmp(name, "trie");
  auto it = e->dtaps.find(name);
  if ((trie && e->dtap_trie.empty()) || (!forms && !trie && it == e->dtaps.end())) {
    if (!strcmp(name, "logits") && e->dtap_pos >= 0 && e->dtap_rows > LOGIT_SLAB)
      set_error(w + "logits are not kept for " + std::to_string(e->dtap_rows) + " trie rows: they exist one slab of " +
                std::to_string(LOGIT_SLAB) + " rows at a time");
    else
      set_error(w + "no tap named " + name + " was kept by the last decoder pass (see rvb_set_decoder_tap)");
    return E_STATE;
  }
  const size_t n = forms ? e->dtap_forms.size() + 1 : dims ? 14 : trie ? e->dtap_trie.size() : it->second.elems;
  if (capacity < (int64_t)n) {
    set_error(w + name + " holds " + std::to_string(n) + " values, the buffer " + std::to_string(capacity));
    return E_ARG;
  }
  if (forms) {
    out[0] = (float)e->dtap_forms.size();
    for (size_t i = 0; i < e->dtap_forms.size(); ++i) out[1 + i] = e->dtap_forms[i];
    return OK;
  }
  if (trie) { memcpy(out, e->dtap_trie.data(), n * 4); return OK; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
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

}  // extern "C"
