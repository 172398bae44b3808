// librvb engine, CTC lattices: forced alignment (chain, wildcard, graph), full-sum scoring (chain, graph) and phrase search over the
// log-prob slabs of the encoded batch.
#include "engine_impl.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rvb {

// Forced alignment (ctc_utils.py:105-161 / bin/alignment.py:233-242).  The log-probs exist one LOGIT_SLAB of rows at a time, exactly as
// rvb_encode produces them (run_gemm on the CTC head + logsoftmax_topk with its lp output, no blank penalty); the Viterbi kernel
// consumes a slab before the next one overwrites it and carries alpha in HBM.  Token confidences need lp[t][label[t]] along the path,
// which is known only after the back-trace: a second sweep of the slabs gathers those T values.
static int align_slab(rvb_engine* e, int r0, int rows) {
  const int d = e->cfg.d_model, V = e->cfg.vocab, Vld = (V + 3) & ~3;
  Scope sc(e, "ctc_align_lp");
  RVB_TRY(run_gemm(e, (const char*)e->enc_out.p + (size_t)r0 * d * dt_size(e->dtype), d, e->ctc, e->logits.p, Vld, rows, true));
  return logsoftmax_topk(e->stream, e->logits.as<float>(), rows, V, Vld, 1, 0.f, e->cfg.blank_id, e->align_tv.as<float>(),
                         e->align_ti.as<int>(), e->align_lp.as<float>());
}

// The lattice entry points (rvb_ctc_align, _align_wild, _align_graph, _score, _find) begin alike once their own arguments are checked:
// align_seq_rows, the driver's plan() (so every refusal comes before any device work), align_workspace, the driver's begin().
// the log-prob rows of each sequence: the valid encoder frames of its chunks, in order
static int align_seq_rows(rvb_engine* e, const char* who, const int32_t* first_chunk, const int32_t* n_chunks, int n_seq,
                          std::vector<std::vector<int32_t>>* seq_rows) {
  if (e->B <= 0) { set_error(std::string(who) + " before rvb_encode"); return E_STATE; }
  seq_rows->assign(n_seq, {});
  for (int i = 0; i < n_seq; ++i) {
    if (first_chunk[i] < 0 || n_chunks[i] < 1 || (int64_t)first_chunk[i] + n_chunks[i] > e->B) {
      set_error(std::string(who) + ": sequence " + std::to_string(i) + ": chunk range outside the encoded batch of " + std::to_string(e->B) + " chunks");
      return E_ARG;
    }
    for (int c = first_chunk[i]; c < first_chunk[i] + n_chunks[i]; ++c)
      for (int t = 0; t < e->enc_lens[c]; ++t) (*seq_rows)[i].push_back(c * e->T2 + t);
  }
  return OK;
}
// the slabs rvb_encode computed its log-probs in (per slice of the batch, LOGIT_SLAB rows at a time): the same GEMM launches, so
// the same bits as the top-k the searches saw
static std::vector<std::pair<int, int>> align_slabs(const rvb_engine* e) {
  std::vector<std::pair<int, int>> slabs;
  auto add_range = [&](int row0, int m) { for (int r0 = 0; r0 < m; r0 += LOGIT_SLAB) slabs.push_back({row0 + r0, std::min(LOGIT_SLAB, m - r0)}); };
  if (e->slices.empty()) add_range(0, e->B * e->T2);
  for (const auto& sl : e->slices) add_range(sl.c0 * e->T2, sl.nb * e->T2);
  return slabs;
}
// the device side of the beginning: the encoded batch is waited for, the slab buffers exist, *slabs = the slabs to sweep
static int align_workspace(rvb_engine* e, std::vector<std::pair<int, int>>* slabs) {
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(wait_slices(e, -1));
  const int V = e->cfg.vocab, Vld = (V + 3) & ~3, slab = std::min(LOGIT_SLAB, e->B * e->T2);
  RVB_TRY(e->logits.ensure((size_t)LOGIT_SLAB * Vld * 4));
  RVB_TRY(e->align_lp.ensure((size_t)slab * V * 4));
  RVB_TRY(e->align_tv.ensure((size_t)slab * 4));
  RVB_TRY(e->align_ti.ensure((size_t)slab * 4));
  *slabs = align_slabs(e);
  return OK;
}

// lp[t][label[t]] of every frame of every lattice (seq: frame_off and T into rows / lab): the slabs once more, one gather_pairs per
// slab.  A wildcard frame's emission is the row maximum, what it emitted less the bias.
template <typename Seq>
static int align_emissions(rvb_engine* e, const std::vector<std::pair<int, int>>& slabs, const std::vector<Seq>& seq,
                           const std::vector<int32_t>& h_rows, const std::vector<int32_t>& lab, bool has_wild, std::vector<float>* emit_out) {
  const int V = e->cfg.vocab, blank = e->cfg.blank_id;
  std::vector<float>& emit = *emit_out;
  emit.resize(lab.size());
  std::vector<int32_t> grow, gcol, gidx;
  std::vector<float> gout, wrow;
  for (const auto& [r0, rows] : slabs) {
    grow.clear(); gcol.clear(); gidx.clear();
    for (const Seq& q : seq) {
      const int frame_off = q.frame_off, T = q.T;
      const int32_t* rw = h_rows.data() + frame_off;
      for (int f = (int)(std::lower_bound(rw, rw + T, r0) - rw); f < T && rw[f] < r0 + rows; ++f) {
        const int32_t l = lab[frame_off + f];
        grow.push_back(rw[f] - r0); gcol.push_back(l == RVB_CTC_WILDCARD ? blank : l); gidx.push_back(frame_off + f);
      }
    }
    if (grow.empty()) continue;
    RVB_TRY(align_slab(e, r0, rows));
    RVB_TRY(upload_i32(e, e->align_row, grow.data(), grow.size()));
    RVB_TRY(upload_i32(e, e->align_col, gcol.data(), gcol.size()));
    RVB_TRY(e->align_out.ensure(grow.size() * 4));
    RVB_TRY(gather_pairs(e->stream, e->align_lp.as<float>(), (size_t)V, e->align_row.as<int>(), e->align_col.as<int>(), (int)grow.size(),
                         e->align_out.as<float>()));
    gout.resize(grow.size());
    RVB_HIP_CHECK(hipMemcpyAsync(gout.data(), e->align_out.p, grow.size() * 4, hipMemcpyDeviceToHost, e->stream));
    if (has_wild) {
      wrow.resize(rows);
      RVB_HIP_CHECK(hipMemcpyAsync(wrow.data(), e->align_tv.p, (size_t)rows * 4, hipMemcpyDeviceToHost, e->stream));
    }
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));     // also: grow / gcol may be rewritten
    for (size_t k = 0; k < gidx.size(); ++k) emit[gidx[k]] = lab[gidx[k]] == RVB_CTC_WILDCARD ? wrow[grow[k]] : gout[k];
  }
  return OK;
}

// One sweep over the slabs, in row order or backwards.  A slab that holds a frame of the driver's sequences is computed (align_slab:
// one GEMM, one log-softmax) and handed to advance(r0, rows) under the profile name `name`; a slab that holds none costs nothing.
template <typename Driver, typename Advance>
static int sweep_slabs(rvb_engine* e, const std::vector<std::pair<int, int>>& slabs, bool descending, const char* name, const Driver& d,
                       Advance advance) {
  for (size_t i = 0; i < slabs.size(); ++i) {
    const auto& [r0, rows] = slabs[descending ? slabs.size() - 1 - i : i];
    if (!d.touches(r0, rows)) continue;
    RVB_TRY(align_slab(e, r0, rows));
    Scope sc(e, name);
    RVB_TRY(advance(r0, rows));
  }
  return OK;
}

// The forward sweep and the back-trace of either aligner (align_tv: the row maxima a wildcard emits): the state of every frame and
// the score of every lattice.
template <typename Aligner>
static int align_sweep(rvb_engine* e, const std::vector<std::pair<int, int>>& slabs, const char* name, Aligner& al, float bias,
                       std::vector<int32_t>* states, std::vector<float>* score) {
  RVB_TRY(sweep_slabs(e, slabs, false, name, al, [&](int r0, int rows) {
    return al.advance(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, rows, e->align_tv.as<float>(), bias);
  }));
  states->resize((size_t)al.total_frames);
  score->resize(al.seq.size());
  Scope sc(e, name);
  return al.finish(e->stream, states->data(), score->data());
}

// The runs of equal values in id[frame_off .. frame_off + T): the state, or the node, of each frame of one lattice's best path.
// slot(value) says where the outputs of a run go (< 0: a blank's run, which has none).  A run yields its first and last frame and,
// from emit (lp[t][label[t]]; filled when peak or confidence is asked for), the frame of its largest emission and that probability.
template <typename Slot>
static void run_outputs(const std::vector<int32_t>& id, const std::vector<float>& emit, int frame_off, int T, Slot slot, int32_t* begin,
                        int32_t* end, int32_t* peak, float* confidence) {
  for (int t = 0; t < T;) {
    const int v = id[frame_off + t];
    int t1 = t;
    while (t1 + 1 < T && id[frame_off + t1 + 1] == v) ++t1;
    const int k = slot(v);
    if (k >= 0) {
      if (begin) begin[k] = t;
      if (end) end[k] = t1;
      if (peak || confidence) {
        int pk = t;
        for (int u = t + 1; u <= t1; ++u) if (emit[frame_off + u] > emit[frame_off + pk]) pk = u;
        if (peak) peak[k] = pk;
        if (confidence) confidence[k] = std::exp(emit[frame_off + pk]);
      }
    }
    t = t1 + 1;
  }
}

// rvb_ctc_align (wild = false: RVB_CTC_WILDCARD is an id outside the vocabulary) and rvb_ctc_align_wild.  A wildcard emits the row's
// top-1 log-prob, which align_slab already produces: align_tv[r] = max logit - lse and lp[r][v] = logit[v] - lse are the same fp32
// subtraction (softmax_topk.hip), so align_tv[r] IS the maximum of the lp row the aligner reads, bit for bit.
static int ctc_align_impl(const char* who, bool wild, float bias, rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq,
                          const int32_t* first_chunk, const int32_t* n_chunks, int32_t* labels, int32_t* begin, int32_t* end,
                          int32_t* peak, float* confidence, float* score) {
  static_assert(CTC_ALIGN_MAX_TOKENS == RVB_CTC_ALIGN_MAX_TOKENS && CTC_ALIGN_MAX_FRAMES == RVB_CTC_ALIGN_MAX_FRAMES, "caps of rvb.h");
  const std::string w(who);
  if (!e) { set_error(w + ": null engine"); return E_ARG; }
  if (!tokens || !tok_lens || !first_chunk || !n_chunks || n_seq <= 0) { set_error(w + ": null argument or n_seq <= 0"); return E_ARG; }
  if (wild && !(std::isfinite(bias) && bias <= 0.f)) { set_error(w + ": wildcard_bias must be finite and <= 0"); return E_ARG; }
  const int V = e->cfg.vocab, blank = e->cfg.blank_id;
  CtcAligner& al = e->aligner;
  std::vector<std::vector<int32_t>> seq_rows;
  RVB_TRY(align_seq_rows(e, who, first_chunk, n_chunks, n_seq, &seq_rows));
  RVB_TRY(al.plan(who, tokens, tok_lens, n_seq, seq_rows, V, blank, wild));
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  RVB_TRY(al.begin(e->stream));
  std::vector<int32_t> states;
  std::vector<float> sc_host;
  RVB_TRY(align_sweep(e, slabs, "ctc_viterbi", al, bias, &states, &sc_host));
  if (score) memcpy(score, sc_host.data(), (size_t)n_seq * 4);
  std::vector<int32_t> lab(states.size());
  for (int i = 0; i < n_seq; ++i) {
    const VitSeq& q = al.seq[i];
    for (int t = 0; t < q.T; ++t) {
      const int st = states[q.frame_off + t];
      lab[q.frame_off + t] = (st & 1) ? tokens[q.tok_off + (st >> 1)] : blank;   // a wildcard's state: RVB_CTC_WILDCARD
    }
  }
  if (labels) memcpy(labels, lab.data(), lab.size() * 4);
  if (!begin && !end && !peak && !confidence) return OK;
  std::vector<float> emit;
  if (peak || confidence) RVB_TRY(align_emissions(e, slabs, al.seq, al.h_rows, lab, al.has_wild, &emit));
  for (const VitSeq& q : al.seq)                   // a run is a state; a token state's outputs go to its token
    run_outputs(states, emit, q.frame_off, q.T, [&](int st) { return (st & 1) ? q.tok_off + (st >> 1) : -1; }, begin, end, peak, confidence);
  return OK;
}

}  // namespace rvb

using namespace rvb;

extern "C" {

int rvb_ctc_align_limits(int32_t* max_tokens, int32_t* max_frames) {
  if (max_tokens) *max_tokens = CTC_ALIGN_MAX_TOKENS;
  if (max_frames) *max_frames = CTC_ALIGN_MAX_FRAMES;
  return OK;
}

int rvb_ctc_align(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* first_chunk,
                  const int32_t* n_chunks, int32_t* labels, int32_t* begin, int32_t* end, int32_t* peak, float* confidence, float* score) {
  return ctc_align_impl("rvb_ctc_align", false, 0.f, e, tokens, tok_lens, n_seq, first_chunk, n_chunks, labels, begin, end, peak,
                        confidence, score);
}
int rvb_ctc_align_wild(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* first_chunk,
                       const int32_t* n_chunks, float wildcard_bias, int32_t* labels, int32_t* begin, int32_t* end, int32_t* peak,
                       float* confidence, float* score) {
  return ctc_align_impl("rvb_ctc_align_wild", true, wildcard_bias, e, tokens, tok_lens, n_seq, first_chunk, n_chunks, labels, begin,
                        end, peak, confidence, score);
}

// Long-form alignment (ctc_viterbi_window.hip): one lattice over several encoded batches.  feed sweeps the slabs of the encoded batch
// exactly as align_sweep does (align_slabs, then align_slab per slab: the log-prob bits the searches saw) and hands each to the
// windowed driver, which is a member of its own: the calls above and below stay usable between begin and finish.
static void long_batch_rows(const rvb_engine* e, std::vector<int32_t>* rows) {
  rows->clear();
  for (int c = 0; c < e->B; ++c)
    for (int t = 0; t < e->enc_lens[c]; ++t) rows->push_back(c * e->T2 + t);
}

int rvb_ctc_align_long_limits(int32_t* max_frames, int32_t* max_window_states, int32_t* default_window_states) {
  if (max_frames) *max_frames = CTC_ALIGN_MAX_FRAMES;
  if (max_window_states) *max_window_states = CTC_WINDOW_MAX_STATES;
  if (default_window_states) *default_window_states = CTC_WINDOW_DEFAULT_STATES;
  return OK;
}

int rvb_ctc_align_long_begin(rvb_engine* e, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states,
                             float wildcard_bias) {
  const char* who = "rvb_ctc_align_long_begin";
  if (!e) { set_error("rvb_ctc_align_long_begin: null engine"); return E_ARG; }
  CtcWindowAligner& al = e->long_aligner;
  al.open = false;                                 // begin while a lattice is open replaces it, also when this one is refused
  RVB_TRY(al.plan(who, tokens, n_tokens, total_frames, window_states, e->cfg.vocab, e->cfg.blank_id, true, wildcard_bias));
  RVB_HIP_CHECK(hipSetDevice(e->device));
  return al.begin(e->stream);
}

int rvb_ctc_align_long_feed(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_align_long_feed: null engine"); return E_ARG; }
  CtcWindowAligner& al = e->long_aligner;
  if (!al.open) { set_error("rvb_ctc_align_long_feed before rvb_ctc_align_long_begin"); return E_STATE; }
  if (e->B <= 0) { set_error("rvb_ctc_align_long_feed before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(al.batch(e->stream, rows));              // E_STATE when the batch holds more frames than the lattice has left
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  return sweep_slabs(e, slabs, false, "ctc_viterbi_window", al, [&](int r0, int nrows) {
    return al.advance(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, nrows, e->align_tv.as<float>());
  });
}

int rvb_ctc_align_long_finish(rvb_engine* e, int32_t* labels, int32_t* begin, int32_t* end, float* score, int32_t* min_margin) {
  if (!e) { set_error("rvb_ctc_align_long_finish: null engine"); return E_ARG; }
  CtcWindowAligner& al = e->long_aligner;
  if (!al.open) { set_error("rvb_ctc_align_long_finish before rvb_ctc_align_long_begin"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  std::vector<int32_t> states((size_t)al.T);
  {
    Scope sc(e, "ctc_viterbi_window");
    RVB_TRY(al.finish(e->stream, states.data(), score, min_margin));
  }
  if (labels)
    for (int t = 0; t < al.T; ++t) labels[t] = (states[t] & 1) ? al.h_tokens[states[t] >> 1] : e->cfg.blank_id;
  if (begin || end) {
    const std::vector<float> no_emit;
    run_outputs(states, no_emit, 0, al.T, [](int st) { return (st & 1) ? (st >> 1) : -1; }, begin, end, nullptr, nullptr);
  }
  return OK;
}

int rvb_ctc_align_long_emissions(rvb_engine* e, const int32_t* labels, int n_frames, float* emit_out) {
  const char* who = "rvb_ctc_align_long_emissions";
  if (!e) { set_error("rvb_ctc_align_long_emissions: null engine"); return E_ARG; }
  if (!labels || !emit_out) { set_error("rvb_ctc_align_long_emissions: null argument"); return E_ARG; }
  if (e->B <= 0) { set_error("rvb_ctc_align_long_emissions before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  if (n_frames != (int)rows.size()) {
    set_error(std::string(who) + ": n_frames " + std::to_string(n_frames) + " is not the " + std::to_string(rows.size()) +
              " valid frames of the encoded batch");
    return E_ARG;
  }
  bool has_wild = false;
  for (int t = 0; t < n_frames; ++t) {
    if (labels[t] == RVB_CTC_WILDCARD) { has_wild = true; continue; }
    if (labels[t] < 0 || labels[t] >= e->cfg.vocab) {
      set_error(std::string(who) + ": label " + std::to_string(labels[t]) + " of frame " + std::to_string(t) + " outside [0, " +
                std::to_string(e->cfg.vocab) + ")");
      return E_ARG;
    }
  }
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  VitSeq q{};
  q.T = n_frames;
  const std::vector<VitSeq> seq(1, q);
  const std::vector<int32_t> lab(labels, labels + n_frames);
  std::vector<float> emit;
  RVB_TRY(align_emissions(e, slabs, seq, rows, lab, has_wild, &emit));
  memcpy(emit_out, emit.data(), (size_t)n_frames * 4);
  return OK;
}

int rvb_ctc_align_long_end(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_align_long_end: null engine"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  e->long_aligner.release();
  return OK;
}

// Long-form full-sum score (ctc_fb_window.hip): rvb_ctc_score's two sweeps inside the aligner's moving window, one lattice over
// several encoded batches.  feed sweeps the slabs of the encoded batch in ascending order, feed_back the same slabs in descending
// order (the CTC head is recomputed, as for rvb_ctc_score's backward sweep).  The driver is a member of its own: the long aligner,
// the one-batch calls and the search stay usable between begin and finish.
int rvb_ctc_score_long_begin(rvb_engine* e, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states, int posteriors) {
  const char* who = "rvb_ctc_score_long_begin";
  if (!e) { set_error("rvb_ctc_score_long_begin: null engine"); return E_ARG; }
  CtcWindowScorer& sc = e->long_scorer;
  sc.open = false;                                 // begin while a lattice is open replaces it, also when this one is refused
  RVB_TRY(sc.plan(who, tokens, n_tokens, total_frames, window_states, e->cfg.vocab, e->cfg.blank_id));
  RVB_HIP_CHECK(hipSetDevice(e->device));
  return sc.begin(e->stream, posteriors != 0);
}

int rvb_ctc_score_long_feed(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_score_long_feed: null engine"); return E_ARG; }
  CtcWindowScorer& sc = e->long_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_long_feed before rvb_ctc_score_long_begin"); return E_STATE; }
  if (e->B <= 0) { set_error("rvb_ctc_score_long_feed before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(sc.batch(e->stream, rows));              // E_STATE when the batch holds more frames than the lattice has left
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  return sweep_slabs(e, slabs, false, "ctc_fb_window_forward", sc, [&](int r0, int nrows) {
    return sc.advance(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, nrows);
  });
}

int rvb_ctc_score_long_loglik(rvb_engine* e, double* loglik) {
  if (!e) { set_error("rvb_ctc_score_long_loglik: null engine"); return E_ARG; }
  if (!loglik) { set_error("rvb_ctc_score_long_loglik: null argument"); return E_ARG; }
  CtcWindowScorer& sc = e->long_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_long_loglik before rvb_ctc_score_long_begin"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  Scope t(e, "ctc_fb_window_forward");
  return sc.finish_forward(e->stream, loglik);
}

int rvb_ctc_score_long_feed_back(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_score_long_feed_back: null engine"); return E_ARG; }
  CtcWindowScorer& sc = e->long_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_long_feed_back before rvb_ctc_score_long_begin"); return E_STATE; }
  if (!sc.post) { set_error("rvb_ctc_score_long_feed_back: the lattice was begun without posteriors"); return E_STATE; }
  if (!sc.forward_done) { set_error("rvb_ctc_score_long_feed_back before rvb_ctc_score_long_loglik"); return E_STATE; }
  if (e->B <= 0) { set_error("rvb_ctc_score_long_feed_back before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(sc.batch_backward(e->stream, rows));     // E_STATE unless the batch is the one the forward sweep saw at this position
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  return sweep_slabs(e, slabs, true, "ctc_fb_window_backward", sc, [&](int r0, int nrows) {
    return sc.advance_backward(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, nrows);
  });
}

int rvb_ctc_score_long_finish(rvb_engine* e, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  if (!e) { set_error("rvb_ctc_score_long_finish: null engine"); return E_ARG; }
  CtcWindowScorer& sc = e->long_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_long_finish before rvb_ctc_score_long_begin"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  Scope t(e, "ctc_fb_window_backward");
  return sc.finish_backward(e->stream, occupancy, mean_frame, peak_post, peak_frame);
}

int rvb_ctc_score_long_end(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_score_long_end: null engine"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  e->long_scorer.release();
  return OK;
}

// Alignment over token graphs (ctc_graph.hip): the slabs, the wildcard's emission and the second sweep for the confidences are those
// of ctc_align_impl; what differs is the lattice and that the per-token outputs follow the chosen path.
int rvb_ctc_align_graph_limits(int32_t* max_nodes, int32_t* max_in_degree, int32_t* max_arcs, int32_t* max_frames) {
  if (max_nodes) *max_nodes = CTC_GRAPH_MAX_NODES;
  if (max_in_degree) *max_in_degree = CTC_GRAPH_MAX_IN_DEGREE;
  if (max_arcs) *max_arcs = CTC_GRAPH_MAX_ARCS;
  if (max_frames) *max_frames = CTC_ALIGN_MAX_FRAMES;
  return OK;
}

int rvb_ctc_align_graph(rvb_engine* e, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds,
                        const uint8_t* is_final, int n_seq, const int32_t* first_chunk, const int32_t* n_chunks, float wildcard_bias,
                        int32_t* labels, int32_t* frame_node, int32_t* path_len, int32_t* path_nodes, int32_t* begin, int32_t* end,
                        int32_t* peak, float* confidence, float* score) {
  static_assert(CTC_GRAPH_MAX_NODES == RVB_CTC_GRAPH_MAX_NODES && CTC_GRAPH_MAX_IN_DEGREE == RVB_CTC_GRAPH_MAX_IN_DEGREE &&
                CTC_GRAPH_MAX_ARCS == RVB_CTC_GRAPH_MAX_ARCS, "caps of rvb.h");
  const std::string w("rvb_ctc_align_graph");
  if (!e) { set_error(w + ": null engine"); return E_ARG; }
  if (!node_tokens || !n_nodes || !pred_off || !preds || !is_final || !first_chunk || !n_chunks || n_seq <= 0) {
    set_error(w + ": null argument or n_seq <= 0");
    return E_ARG;
  }
  if (!(std::isfinite(wildcard_bias) && wildcard_bias <= 0.f)) { set_error(w + ": wildcard_bias must be finite and <= 0"); return E_ARG; }
  const int V = e->cfg.vocab, blank = e->cfg.blank_id;
  CtcGraphAligner& al = e->graph_aligner;
  std::vector<std::vector<int32_t>> seq_rows;
  RVB_TRY(align_seq_rows(e, w.c_str(), first_chunk, n_chunks, n_seq, &seq_rows));
  RVB_TRY(al.plan(w.c_str(), node_tokens, n_nodes, pred_off, preds, is_final, n_seq, seq_rows, V, blank));
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  RVB_TRY(al.begin(e->stream));
  std::vector<int32_t> states;
  std::vector<float> sc_host;
  RVB_TRY(align_sweep(e, slabs, "ctc_graph", al, wildcard_bias, &states, &sc_host));
  std::vector<int32_t> lab(states.size()), node(states.size());
  for (int i = 0; i < n_seq; ++i) {
    const GraphSeq& q = al.seq[i];
    for (int t = 0; t < q.T; ++t) {
      const int st = states[q.frame_off + t], j = (st >> 1) - 1;
      node[q.frame_off + t] = (st & 1) ? j : -1;
      lab[q.frame_off + t] = (st & 1) ? node_tokens[q.node_off + j] : blank;
    }
  }
  std::vector<float> emit;
  if (peak || confidence) RVB_TRY(align_emissions(e, slabs, al.seq, al.h_rows, lab, al.has_wild, &emit));
  // nothing was written so far: a refusal leaves every output untouched
  if (score) memcpy(score, sc_host.data(), (size_t)n_seq * 4);
  if (labels) memcpy(labels, lab.data(), lab.size() * 4);
  if (frame_node) memcpy(frame_node, node.data(), node.size() * 4);
  for (int i = 0; i < n_seq; ++i) {
    const GraphSeq& q = al.seq[i];
    int n_path = 0;
    auto next_on_path = [&](int j) {               // a run is a node; its outputs go to the next position of the chosen path
      if (j < 0) return -1;
      const int k = q.node_off + n_path++;
      if (path_nodes) path_nodes[k] = j;
      return k;
    };
    run_outputs(node, emit, q.frame_off, q.T, next_on_path, begin, end, peak, confidence);
    if (path_len) path_len[i] = n_path;
  }
  return OK;
}

// Long-form alignment over a token graph (ctc_graph_window.hip): rvb_ctc_align_long_*'s protocol for ONE graph of any number of
// nodes.  feed sweeps the slabs of the encoded batch as rvb_ctc_align_long_feed does; peaks and confidences come from a second pass
// of encodes through rvb_ctc_align_long_emissions, which needs no open lattice.  The driver is a member of its own: the one-batch
// calls, the long chain calls and the search stay usable between begin and finish.
int rvb_ctc_align_graph_long_limits(int32_t* max_frames, int32_t* max_in_degree, int32_t* max_window_nodes, int32_t* default_window_nodes) {
  if (max_frames) *max_frames = CTC_ALIGN_MAX_FRAMES;
  if (max_in_degree) *max_in_degree = CTC_GRAPH_MAX_IN_DEGREE;
  if (max_window_nodes) *max_window_nodes = CTC_GRAPH_WINDOW_MAX_NODES;
  if (default_window_nodes) *default_window_nodes = CTC_GRAPH_WINDOW_DEFAULT_NODES;
  return OK;
}

int rvb_ctc_align_graph_long_begin(rvb_engine* e, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                   const uint8_t* is_final, int64_t total_frames, int window_nodes, float wildcard_bias) {
  const char* who = "rvb_ctc_align_graph_long_begin";
  if (!e) { set_error("rvb_ctc_align_graph_long_begin: null engine"); return E_ARG; }
  CtcGraphWindowAligner& al = e->long_graph_aligner;
  al.open = false;                                 // begin while a lattice is open replaces it, also when this one is refused
  RVB_TRY(al.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, total_frames, window_nodes, e->cfg.vocab, e->cfg.blank_id,
                  wildcard_bias));
  RVB_HIP_CHECK(hipSetDevice(e->device));
  return al.begin(e->stream);
}

int rvb_ctc_align_graph_long_feed(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_align_graph_long_feed: null engine"); return E_ARG; }
  CtcGraphWindowAligner& al = e->long_graph_aligner;
  if (!al.open) { set_error("rvb_ctc_align_graph_long_feed before rvb_ctc_align_graph_long_begin"); return E_STATE; }
  if (e->B <= 0) { set_error("rvb_ctc_align_graph_long_feed before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(al.batch(e->stream, rows));              // E_STATE when the batch holds more frames than the lattice has left
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  return sweep_slabs(e, slabs, false, "ctc_graph_window", al, [&](int r0, int nrows) {
    return al.advance(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, nrows, e->align_tv.as<float>());
  });
}

int rvb_ctc_align_graph_long_finish(rvb_engine* e, int32_t* labels, int32_t* frame_node, int32_t* path_len, int32_t* path_nodes,
                                    int32_t* begin, int32_t* end, float* score, int32_t* min_margin) {
  if (!e) { set_error("rvb_ctc_align_graph_long_finish: null engine"); return E_ARG; }
  CtcGraphWindowAligner& al = e->long_graph_aligner;
  if (!al.open) { set_error("rvb_ctc_align_graph_long_finish before rvb_ctc_align_graph_long_begin"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  std::vector<int32_t> states((size_t)al.T);
  {
    Scope sc(e, "ctc_graph_window");
    RVB_TRY(al.finish(e->stream, states.data(), score, min_margin));   // a refusal leaves every output untouched
  }
  std::vector<int32_t> node((size_t)al.T);
  for (int t = 0; t < al.T; ++t) {
    const int st = states[t], j = (st >> 1) - 1;
    node[t] = (st & 1) ? j : -1;
    if (labels) labels[t] = (st & 1) ? al.h_tokens[j] : e->cfg.blank_id;
  }
  if (frame_node) memcpy(frame_node, node.data(), node.size() * 4);
  const std::vector<float> no_emit;
  int n_path = 0;
  auto next_on_path = [&](int j) {                 // a run is a node; its outputs go to the next position of the chosen path
    if (j < 0) return -1;
    const int k = n_path++;
    if (path_nodes) path_nodes[k] = j;
    return k;
  };
  run_outputs(node, no_emit, 0, al.T, next_on_path, begin, end, nullptr, nullptr);
  if (path_len) *path_len = n_path;
  return OK;
}

int rvb_ctc_align_graph_long_end(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_align_graph_long_end: null engine"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  e->long_graph_aligner.release();
  return OK;
}

// Long-form full-sum score over a token graph (ctc_graph_fb_window.hip): rvb_ctc_score_long_*'s protocol for ONE graph of any number
// of nodes.  feed sweeps the slabs of the encoded batch in ascending order, feed_back the same slabs in descending order (the CTC head
// is recomputed).  The driver is a member of its own: the one-batch calls, the other long lattices and the search stay usable between
// begin and end.
int rvb_ctc_score_graph_long_limits(int32_t* max_frames, int32_t* max_in_degree, int32_t* max_window_nodes, int32_t* default_window_nodes) {
  if (max_frames) *max_frames = CTC_ALIGN_MAX_FRAMES;
  if (max_in_degree) *max_in_degree = CTC_GRAPH_MAX_IN_DEGREE;
  if (max_window_nodes) *max_window_nodes = CTC_GRAPH_SCORE_WINDOW_MAX_NODES;
  if (default_window_nodes) *default_window_nodes = CTC_GRAPH_SCORE_WINDOW_DEFAULT_NODES;
  return OK;
}

int rvb_ctc_score_graph_long_begin(rvb_engine* e, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                   const uint8_t* is_final, int64_t total_frames, int window_nodes, int posteriors) {
  const char* who = "rvb_ctc_score_graph_long_begin";
  if (!e) { set_error("rvb_ctc_score_graph_long_begin: null engine"); return E_ARG; }
  CtcGraphWindowScorer& sc = e->long_graph_scorer;
  sc.open = false;                                 // begin while a lattice is open replaces it, also when this one is refused
  RVB_TRY(sc.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, total_frames, window_nodes, e->cfg.vocab, e->cfg.blank_id,
                  posteriors != 0));
  RVB_HIP_CHECK(hipSetDevice(e->device));
  return sc.begin(e->stream);
}

int rvb_ctc_score_graph_long_feed(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_score_graph_long_feed: null engine"); return E_ARG; }
  CtcGraphWindowScorer& sc = e->long_graph_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_graph_long_feed before rvb_ctc_score_graph_long_begin"); return E_STATE; }
  if (e->B <= 0) { set_error("rvb_ctc_score_graph_long_feed before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(sc.batch(e->stream, rows));              // E_STATE when the batch holds more frames than the lattice has left
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  return sweep_slabs(e, slabs, false, "ctc_graph_fb_window_forward", sc, [&](int r0, int nrows) {
    return sc.advance(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, nrows);
  });
}

int rvb_ctc_score_graph_long_loglik(rvb_engine* e, double* loglik) {
  if (!e) { set_error("rvb_ctc_score_graph_long_loglik: null engine"); return E_ARG; }
  if (!loglik) { set_error("rvb_ctc_score_graph_long_loglik: null argument"); return E_ARG; }
  CtcGraphWindowScorer& sc = e->long_graph_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_graph_long_loglik before rvb_ctc_score_graph_long_begin"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  Scope t(e, "ctc_graph_fb_window_forward");
  return sc.loglik(e->stream, loglik);
}

int rvb_ctc_score_graph_long_feed_back(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_score_graph_long_feed_back: null engine"); return E_ARG; }
  CtcGraphWindowScorer& sc = e->long_graph_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_graph_long_feed_back before rvb_ctc_score_graph_long_begin"); return E_STATE; }
  if (!sc.post) { set_error("rvb_ctc_score_graph_long_feed_back: the lattice was begun without posteriors"); return E_STATE; }
  if (!sc.forward_done) { set_error("rvb_ctc_score_graph_long_feed_back before rvb_ctc_score_graph_long_loglik"); return E_STATE; }
  if (e->B <= 0) { set_error("rvb_ctc_score_graph_long_feed_back before rvb_encode"); return E_STATE; }
  std::vector<int32_t> rows;
  long_batch_rows(e, &rows);
  RVB_HIP_CHECK(hipSetDevice(e->device));
  RVB_TRY(sc.batch_back(e->stream, rows));         // E_STATE unless the batch is the one the forward sweep saw at this position
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  return sweep_slabs(e, slabs, true, "ctc_graph_fb_window_backward", sc, [&](int r0, int nrows) {
    return sc.advance_back(e->stream, e->align_lp.as<float>(), e->cfg.vocab, r0, nrows);
  });
}

int rvb_ctc_score_graph_long_finish(rvb_engine* e, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  if (!e) { set_error("rvb_ctc_score_graph_long_finish: null engine"); return E_ARG; }
  CtcGraphWindowScorer& sc = e->long_graph_scorer;
  if (!sc.open) { set_error("rvb_ctc_score_graph_long_finish before rvb_ctc_score_graph_long_begin"); return E_STATE; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  Scope t(e, "ctc_graph_fb_window_backward");
  return sc.finish(e->stream, visit, occupancy, mean_frame, peak_post, peak_frame);
}

int rvb_ctc_score_graph_long_end(rvb_engine* e) {
  if (!e) { set_error("rvb_ctc_score_graph_long_end: null engine"); return E_ARG; }
  RVB_HIP_CHECK(hipSetDevice(e->device));
  e->long_graph_scorer.release();
  return OK;
}

// Full-sum score (CTC.forward, transformer/ctc.py:65-104) over the same slabs: a forward sweep, and for per-token outputs the slabs
// once more in descending order for the backward sweep (the CTC head is recomputed, as for the alignment's confidences).
int rvb_ctc_score(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const int32_t* first_chunk,
                  const int32_t* n_chunks, double* loglik, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  if (!e) { set_error("rvb_ctc_score: null engine"); return E_ARG; }
  if (!tokens || !tok_lens || !first_chunk || !n_chunks || !loglik || n_seq <= 0) { set_error("rvb_ctc_score: null argument or n_seq <= 0"); return E_ARG; }
  const char* who = "rvb_ctc_score";
  const int V = e->cfg.vocab;
  CtcScorer& sc = e->scorer;
  const bool post = occupancy || mean_frame || peak_post || peak_frame;
  std::vector<std::vector<int32_t>> seq_rows;
  RVB_TRY(align_seq_rows(e, who, first_chunk, n_chunks, n_seq, &seq_rows));
  RVB_TRY(sc.plan(who, tokens, tok_lens, n_seq, seq_rows, V, e->cfg.blank_id));
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  RVB_TRY(sc.begin(e->stream, post));
  RVB_TRY(sweep_slabs(e, slabs, false, "ctc_forward", sc.lat,
                      [&](int r0, int rows) { return sc.advance(e->stream, e->align_lp.as<float>(), V, r0, rows); }));
  {
    Scope t(e, "ctc_forward");
    RVB_TRY(sc.finish_forward(e->stream, loglik));
  }
  if (!post) return OK;
  RVB_TRY(sweep_slabs(e, slabs, true, "ctc_backward", sc.lat,
                      [&](int r0, int rows) { return sc.advance_backward(e->stream, e->align_lp.as<float>(), V, r0, rows); }));
  Scope t(e, "ctc_backward");
  return sc.finish_backward(e->stream, occupancy, mean_frame, peak_post, peak_frame);
}

// Full-sum score over token graphs (ctc_graph_score.hip): rvb_ctc_score's two sweeps on the lattices of rvb_ctc_align_graph.  Nothing
// is written before the last step has succeeded: a refusal leaves every output untouched.
int rvb_ctc_score_graph(rvb_engine* e, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds,
                        const uint8_t* is_final, int n_seq, const int32_t* first_chunk, const int32_t* n_chunks, double* loglik,
                        float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  const char* who = "rvb_ctc_score_graph";
  if (!e) { set_error("rvb_ctc_score_graph: null engine"); return E_ARG; }
  if (!node_tokens || !n_nodes || !pred_off || !preds || !is_final || !first_chunk || !n_chunks || !loglik || n_seq <= 0) {
    set_error("rvb_ctc_score_graph: null argument or n_seq <= 0");
    return E_ARG;
  }
  const int V = e->cfg.vocab;
  CtcGraphScorer& sc = e->graph_scorer;
  const bool post = visit || occupancy || mean_frame || peak_post || peak_frame;
  std::vector<std::vector<int32_t>> seq_rows;
  RVB_TRY(align_seq_rows(e, who, first_chunk, n_chunks, n_seq, &seq_rows));
  RVB_TRY(sc.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, n_seq, seq_rows, V, e->cfg.blank_id, post));
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  RVB_TRY(sc.begin(e->stream));
  RVB_TRY(sweep_slabs(e, slabs, false, "ctc_graph_forward", sc.lat,
                      [&](int r0, int rows) { return sc.advance(e->stream, e->align_lp.as<float>(), V, r0, rows); }));
  std::vector<double> ll((size_t)n_seq);
  {
    Scope t(e, "ctc_graph_forward");
    RVB_TRY(sc.finish_forward(e->stream, ll.data()));
  }
  if (post) {
    RVB_TRY(sweep_slabs(e, slabs, true, "ctc_graph_backward", sc.lat,
                        [&](int r0, int rows) { return sc.advance_backward(e->stream, e->align_lp.as<float>(), V, r0, rows); }));
    Scope t(e, "ctc_graph_backward");
    RVB_TRY(sc.finish_backward(e->stream, visit, occupancy, mean_frame, peak_post, peak_frame));
  }
  memcpy(loglik, ll.data(), (size_t)n_seq * 8);
  return OK;
}

// Phrase search (csrc/ctc_find.hip) over the same slabs: align_slab leaves the log-probs in align_lp and each row's maximum in
// align_tv (the same fp32 subtraction, see ctc_align_impl), which is all the kernel reads.  Everything is checked before any device work.
int rvb_ctc_find(rvb_engine* e, const int32_t* tokens, const int32_t* tok_lens, int n_phrases, const float* threshold,
                 const int32_t* first_chunk, const int32_t* n_chunks, int n_seq, int max_candidates, int max_hits, int32_t* n_hits,
                 int32_t* start, int32_t* end, float* score, int64_t* n_candidates) {
  static_assert(CTC_FIND_MAX_TOKENS == RVB_CTC_FIND_MAX_TOKENS, "cap of rvb.h");
  const char* who = "rvb_ctc_find";
  if (!e) { set_error("rvb_ctc_find: null engine"); return E_ARG; }
  if (!tokens || !tok_lens || !threshold || !first_chunk || !n_chunks || !n_hits || !start || !end || !score) {
    set_error("rvb_ctc_find: null argument"); return E_ARG;
  }
  if (n_phrases < 1 || n_seq < 1) { set_error("rvb_ctc_find: need n_phrases >= 1 and n_seq >= 1"); return E_ARG; }
  if (max_candidates < 1 || max_hits < 1) { set_error("rvb_ctc_find: need max_candidates >= 1 and max_hits >= 1"); return E_ARG; }
  const int V = e->cfg.vocab;
  CtcFinder& fd = e->finder;
  std::vector<std::vector<int32_t>> seq_rows;
  RVB_TRY(align_seq_rows(e, who, first_chunk, n_chunks, n_seq, &seq_rows));
  RVB_TRY(fd.plan(who, tokens, tok_lens, n_phrases, threshold, seq_rows, V, e->cfg.blank_id, max_candidates));
  std::vector<std::pair<int, int>> slabs;
  RVB_TRY(align_workspace(e, &slabs));
  RVB_TRY(fd.begin(e->stream));
  RVB_TRY(sweep_slabs(e, slabs, false, "ctc_find", fd, [&](int r0, int rows) {
    return fd.advance(e->stream, e->align_lp.as<float>(), V, r0, rows, e->align_tv.as<float>());
  }));
  return fd.finish(e->stream, max_hits, n_hits, start, end, score, n_candidates);
}

}  // extern "C"
