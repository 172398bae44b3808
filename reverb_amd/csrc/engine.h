// Engine: weights, workspace and orchestration of the Reverb-ASR hot path on one MI355X.
#pragma once
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rvb.h"
#include "ctc_slabs.h"
#include "kernels.h"
#include "search.h"

namespace rvb {

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t n);   // grow-only
  void release();
  template <typename T> T* as() const { return (T*)p; }
};

struct Linear {      // y = x.W^T + b, W packed to the compute dtype [out][in]
  DevBuf w, b;
  int out = 0, in = 0;
  DevBuf w8, wscale;   // fp8 mode: e4m3 copy [out][in] and its per-output-channel scales fp32 [out]
};
// per-tensor scales of the activations an fp8 GEMM reads (value = fp8 * scale), one set per conformer block
struct F8Scales { float in_ffm1 = 1, h_ffm = 1, in_qkv = 1, in_pw1 = 1, in_pw2 = 1, in_ff1 = 1, h_ff = 1; };
struct LNorm { DevBuf g, b; float eps = 1e-5f; };

struct EncLayer {
  Linear ffm1, ffm2, ff1, ff2, qkv, att_out, pw1, pw2, lsl;
  Linear pw1_glu;             // bf16 engine: pw1 with its output rows interleaved (a_0, b_0, a_1, b_1, ...) for the GEMM's ACT_GLU epilogue
  DevBuf pos_keys;            // T [Tpos, d] = linear_pos(pe[:Tpos])
  DevBuf pos_bias;            // bf16 engine: fp32 [heads][Tpos], (pos_bias_v - pos_bias_u) . pos_keys * log2(e)/sqrt(dk) (attention.hip FOLD)
  DevBuf bias_u, bias_v;      // fp32 [h*dk]
  LNorm n_ffm, n_mha, n_conv, n_ff, n_final, n_cnn;
  DevBuf dw_w, dw_b;          // fp32 [K][d] (tap-major), [d]
  bool is_lsl = false;
};
struct DecLayer {
  Linear self_qkv, self_out, src_q, src_kv, src_out, ff1, ff2, lsl;
  LNorm n1, n2, n3;
  bool is_lsl = false;
  DevBuf kvmem;               // T [B*T2][2d]: this layer's keys / values of the encoder output (rescoring)
};
struct Decoder {
  DevBuf embed;               // fp32 [V][d]
  Linear out;
  LNorm after;
  std::vector<DecLayer> layers;
  bool present = false;
  bool kv_ready = false;      // the layers' kvmem hold the current batch (rvb_prepare_rescoring or the first decoder pass)
};

struct ProfEntry { double ms = 0, flops = 0, bytes = 0; int64_t launches = 0; };

struct RescoreResult {
  int best = 0;
  float score = 0.f;
  double confidence = 0.0;
  std::vector<double> tok_conf;
  std::vector<std::vector<float>> logp, rlogp;   // per hyp: len+1 decoder log-probs
};


// Host worker threads kept alive across calls (prefix beam search per slice, trie building): starting 31 threads costs
// about as much as the work of the last, un-overlapped slice.  run(n, fn): fn is executed by n threads, the caller among them.
class HostPool {
 public:
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  void run(unsigned n, const std::function<void()>& fn) {
    if (n <= 1) { fn(); return; }
    {
      std::lock_guard<std::mutex> lk(m_);
      while (th_.size() + 1 < n) th_.emplace_back([this] { loop(); });
      job_ = &fn; want_ = n - 1; started_ = 0; finished_ = 0; ++gen_;
    }
    cv_.notify_all();
    fn();
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [&] { return finished_ == want_; });
    job_ = nullptr;
  }

 private:
  void loop() {
    unsigned long long seen = 0;
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || (gen_ != seen && started_ < want_); });
      if (stop_) return;
      seen = gen_;
      ++started_;
      const std::function<void()>* job = job_;
      lk.unlock();
      (*job)();
      lk.lock();
      if (++finished_ == want_) done_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void()>* job_ = nullptr;
  unsigned want_ = 0, started_ = 0, finished_ = 0;
  unsigned long long gen_ = 0;
  bool stop_ = false;
};

// ---- rescoring: every DISTINCT prefix of a chunk's n-best list is one decoder row (trie.h, engine_decode.hip "rescoring")
struct HypRef { int chunk, idx, len, row0; };      // row0: first of the hypothesis' len+1 (hyp, j) pairs

struct TrieBatch {
  int R = 0, P = 0, max_chunk_rows = 0;            // unique rows, (hyp, j) pairs, most rows of one chunk
  std::vector<int32_t> tok, pos;                   // per row: input token, position
  std::vector<int32_t> path;                       // per hypothesis: the rows of its prefixes 0..len (flat)
  std::vector<int32_t> hq_start, hq_len, hq_pos0, hkv_start, hkv_len;   // per hypothesis: owned rows / path
  std::vector<int32_t> crow_start, crow_len;       // per chunk: its rows (contiguous)
  std::vector<int32_t> tgt_ptr, tgt;               // CSR over rows: the targets asked of a row
  std::vector<int32_t> pair_slot;                  // (hyp, j) pair -> position in tgt / in the gathered log-probs
  std::vector<int32_t> work;                       // self-attention blocks: {hypothesis, first owned query}
};

// ---- forced alignment (ctc_viterbi.hip): the host side of a batch of lattices, shared by rvb_ctc_align and the lab hook.
// plan() validates and lays out (no device work), begin() allocates and uploads, advance() runs the forward kernel over the frames
// whose rows lie in the slab just computed (slabs in row order), finish() back-traces and returns states and scores.
// With allow_wild, plan() accepts RVB_CTC_WILDCARD as a token (a label of its own: it counts towards the caps and, next to another
// wildcard, as a repeat); advance() then needs wmax[nrows], the maximum of each row of the slab, and the per-frame bias <= 0.
// The five drivers below share their slab feed (row checks, frame windows per slab, coverage, descriptor upload): ctc_slabs.h.
struct CtcAligner {
  std::vector<VitSeq> seq;
  std::vector<int32_t> h_tokens, h_rows;
  int max_S = 0, blank = 0;
  bool has_wild = false;                           // some sequence of the plan holds a wildcard: the WILD kernels run
  size_t alpha_floats = 0, bp_bytes = 0;
  int64_t total_frames = 0;
  DevBuf d_tokens, d_rows, d_seqs, d_alpha, d_bp, d_states, d_score;
  // seq_rows[i][f]: the (increasing) log-prob row of frame f of sequence i
  int plan(const char* who, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const std::vector<std::vector<int32_t>>& seq_rows,
           int V, int blank_id, bool allow_wild = false);
  int begin(hipStream_t s);
  bool touches(int r0, int nrows) const { return slab_touches(seq, h_rows, r0, nrows); }
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax = nullptr, float bias = 0.f);
  int finish(hipStream_t s, int32_t* states /* [total_frames] */, float* score /* [n_seq] */);
  void release();
};

// ---- alignment over a token graph (ctc_graph.hip): CtcAligner's plan / begin / touches / advance / finish / release for lattices
// with alternatives, shared by rvb_ctc_align_graph and the lab hook.  plan() takes the graphs as the C ABI does (pred_off: n_nodes + 1
// offsets per sequence, concatenated, within the sequence's predecessors), refuses by sequence and node, and encodes the arcs.
struct CtcGraphAligner {
  std::vector<GraphSeq> seq;
  std::vector<int32_t> h_tokens, h_arc_off, h_finals, h_rows;
  std::vector<uint32_t> h_arcs;
  int max_N = 0, blank = 0;
  bool has_wild = false;                           // some node of the plan is a wildcard: advance() needs the row maxima
  size_t alpha_floats = 0, bp_bytes = 0;
  int64_t total_frames = 0;
  DevBuf d_tokens, d_arc_off, d_arcs, d_finals, d_rows, d_seqs, d_alpha, d_bp, d_states, d_score;
  int plan(const char* who, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds,
           const uint8_t* is_final, int n_seq, const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id);
  int begin(hipStream_t s);
  bool touches(int r0, int nrows) const { return slab_touches(seq, h_rows, r0, nrows); }
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax = nullptr, float bias = 0.f);
  int finish(hipStream_t s, int32_t* states /* [total_frames]: 2 * slot + token bit */, float* score /* [n_seq] */);
  void release();
};

// ---- full-sum scoring (ctc_forward_backward.hip): the host side shared by rvb_ctc_score and the lab hook.  The lattices are the
// aligner's: plan() is CtcAligner::plan (same checks, refusals and layout).  begin() allocates (with posteriors: the alpha rows, or
// E_NOMEM naming their size), advance() runs the forward kernel over a slab (slabs in row order), finish_forward() returns loglik;
// advance_backward() takes the same slabs in descending order, finish_backward() returns the per-token reductions.
struct CtcScorer {
  CtcAligner lat;
  bool post = false;
  DevBuf d_csum, d_loglik, d_llhat, d_coff, d_arows, d_beta, d_z, d_acc;
  int plan(const char* who, const int32_t* tokens, const int32_t* tok_lens, int n_seq, const std::vector<std::vector<int32_t>>& seq_rows,
           int V, int blank_id);
  int begin(hipStream_t s, bool posteriors);
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish_forward(hipStream_t s, double* loglik /* [n_seq] */);
  int advance_backward(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish_backward(hipStream_t s, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame /* per token, nullable */);
  void release();
};


// ---- full-sum scoring over a token graph (ctc_graph_score.hip): the host side shared by rvb_ctc_score_graph and the lab hook, as
// CtcScorer is for chains.  plan() is CtcGraphAligner::plan (same checks, refusals and layout), then refuses wildcards, with
// posteriors an out-degree above the in-degree cap, and a graph no path of which fits the frames; it computes every state's fewest
// frames to a final end (the normaliser's live set) and the transposed arcs.  The sweeps are CtcScorer's.
struct CtcGraphScorer {
  CtcGraphAligner lat;
  bool post = false;
  std::vector<uint32_t> h_rem, h_succs;
  std::vector<int32_t> h_succ_off;
  std::vector<uint8_t> h_fin;
  DevBuf d_rem, d_csum, d_loglik, d_llhat, d_coff, d_arows, d_beta, d_acc, d_succ_off, d_succs, d_fin;
  int plan(const char* who, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds,
           const uint8_t* is_final, int n_seq, const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id, bool posteriors);
  int begin(hipStream_t s);
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish_forward(hipStream_t s, double* loglik /* [n_seq] */);
  int advance_backward(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish_backward(hipStream_t s, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame /* per node, nullable */);
  void release();
};

// ---- phrase search (ctc_find.hip): the host side shared by rvb_ctc_find and the lab hook.  plan() validates and lays out the
// (phrase, sequence) pairs (no device work; E_NOMEM if the candidate buffers cannot fit any device), begin() allocates and uploads
// (E_NOMEM naming the bytes), advance() runs the kernel over the frames whose rows lie in the slab just computed (slabs in row
// order; wmax[nrows] = the maximum of each row of the slab), finish() copies counts and candidates back and suppresses overlapping
// candidates on the host.  A sequence shorter than a phrase is no error: it has no arrival.
struct CtcFinder {
  std::vector<FindSeq> seq;
  std::vector<FindPhrase> phr;
  std::vector<int32_t> h_tokens, h_rows;
  int blank = 0, max_cand = 0;
  DevBuf d_tokens, d_rows, d_seqs, d_phr, d_h, d_st, d_count, d_cend, d_cstart, d_cscore;
  // seq_rows[i][f]: the (increasing) log-prob row of frame f of sequence i; threshold [n_phrases]
  int plan(const char* who, const int32_t* tokens, const int32_t* tok_lens, int n_phrases, const float* threshold,
           const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id, int max_candidates);
  int begin(hipStream_t s);
  bool touches(int r0, int nrows) const { return slab_touches(seq, h_rows, r0, nrows); }
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax);
  // pair p = phrase * n_seq + sequence: n_hits [pairs], start / end / score [pairs][max_hits], n_candidates [pairs] (nullable: all
  // arrivals at or above the threshold, kept or not); raw_* (nullable) [pairs][max_cand]: the kept candidates as the kernel wrote them
  int finish(hipStream_t s, int max_hits, int32_t* n_hits, int32_t* start, int32_t* end, float* score, int64_t* n_candidates,
             int32_t* raw_end = nullptr, int32_t* raw_start = nullptr, float* raw_score = nullptr);
  void release();
};

// ---- long-form alignment (ctc_viterbi_window.hip): ONE lattice of any number of tokens whose frames arrive over several encoded
// batches, shared by rvb_ctc_align_long_* and the lab hook.  Only W consecutive states are alive at a frame (the window); the
// window moves between launches, placed by ctc_window_next_lo from the best state the launch before reported.
// plan() validates in CtcAligner::plan's words (no token cap beyond L <= frames; no device work), begin() allocates (E_NOMEM naming
// the back-pointer bytes) and sets alpha to -inf, batch() takes the log-prob rows of the next frames (one encoded batch), advance()
// runs the kernel over the frames of the batch whose rows lie in the slab (slabs in row order; launches of at most W / 4 frames),
// finish() back-traces: states, score and the path's smallest distance to a window edge that is not the lattice's own.
enum { CTC_WINDOW_MAX_STATES = 32768, CTC_WINDOW_DEFAULT_STATES = 32768 };
// the window of the launch over frames [f0, f1), given the window before and the first-maximum state of the last frame (-1: none)
int ctc_window_next_lo(int S, int T, int W, int f0, int f1, int lo_prev, int best_prev);
struct CtcWindowAligner {
  int L = 0, S = 0, S_pad = 0, T = 0, W = 0, blank = 0;
  bool has_wild = false, open = false;
  float bias = 0.f;
  std::vector<int32_t> h_tokens, h_rows;           // h_rows: the rows of the batch being fed, its first frame is lattice frame fbase
  int fed = 0, fbase = 0;                          // lattice frames advanced so far
  int lo = 0, best = -1;                           // the last launch's window and the best state it reported
  size_t bp_bytes = 0;
  DevBuf d_tokens, d_rows, d_alpha, d_bp, d_lo, d_best, d_states, d_end;
  int plan(const char* who, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states, int V, int blank_id,
           bool allow_wild, float wildcard_bias);
  int begin(hipStream_t s);
  int batch(hipStream_t s, const std::vector<int32_t>& rows);
  bool touches(int r0, int nrows) const;
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax = nullptr);
  int finish(hipStream_t s, int32_t* states /* [T] */, float* score, int32_t* min_margin, int32_t* lo_out = nullptr /* [T] */);
  void release();
};

// ---- long-form full-sum scoring (ctc_fb_window.hip): CtcScorer's two sweeps inside CtcWindowAligner's moving window, shared by
// rvb_ctc_score_long_* and the lab hook.  plan() is CtcWindowAligner::plan without wildcards (no device work), begin() allocates (with
// posteriors: T x W x 4 bytes of alpha rows, or E_NOMEM naming them), batch() / advance() feed the encoded batches in ascending order
// (launches cut as the aligner's; the host keeps every launch's frames, window and reported best state), finish_forward() returns
// loglik; batch_backward() / advance_backward() take the same batches in DESCENDING order, slabs descending within a batch, and replay
// the recorded launches in reverse; finish_backward() returns the per-token reductions.
struct CtcWindowScorer {
  struct Launch { int f0, f1, lo, best; };
  int L = 0, S = 0, S_pad = 0, T = 0, W = 0, blank = 0;
  bool open = false, post = false, forward_done = false;
  std::vector<int32_t> h_tokens, h_rows;           // h_rows: the rows of the batch being fed, its first frame is lattice frame fbase
  std::vector<Launch> launches;                    // the forward launches in order: they tile [0, fed)
  std::vector<int> batches;                        // frames of every forward batch, in order
  int fed = 0, fbase = 0;                          // forward: lattice frames advanced so far
  int lo = 0, best = -1;                           // the last launch's window and the best state it reported
  int back = 0, back_batch = 0, cursor = 0;        // backward: frames still to go, batches still to come, launches below the cursor
  const int32_t* lo_force = nullptr;               // lab hook: the window of launch i, in place of the policy's answer
  int n_force = 0;
  size_t row_bytes = 0;
  DevBuf d_tokens, d_rows, d_alpha, d_seq, d_csum, d_loglik, d_llhat, d_best, d_coff, d_arows, d_beta, d_z, d_acc;
  int plan(const char* who, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states, int V, int blank_id);
  int launch_count(int slab_rows) const;           // launches of a forward sweep fed slab_rows frames at a time (one batch)
  int rows_fit() const;                            // the lab switch RVB_CTC_SCORE_FAKE_NOMEM_ABOVE against the alpha rows; no device work
  int begin(hipStream_t s, bool posteriors);
  int batch(hipStream_t s, const std::vector<int32_t>& rows);
  bool touches(int r0, int nrows) const;
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish_forward(hipStream_t s, double* loglik);
  int batch_backward(hipStream_t s, const std::vector<int32_t>& rows);
  int advance_backward(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish_backward(hipStream_t s, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame /* per token, nullable */);
  void lo_per_frame(int32_t* lo_out /* [fed] */) const;
  void release();
};

// ---- long-form alignment over a token graph (ctc_graph_window.hip): ONE graph of any number of nodes whose frames arrive over
// several encoded batches, shared by rvb_ctc_align_graph_long_* and the lab hook.  Only W consecutive nodes are alive at a frame; the
// window moves between launches, and both the window and the launch's length come from ctc_graph_window_next: an arc of a graph can
// climb many nodes at once, so a launch lasts for as long as the highest node the best partial path can have reached stays inside.
// plan() makes CtcGraphAligner::plan's checks in its words (no node or arc cap; no device work), computes the policy's tables and
// refuses a graph whose shortest reading needs more frames than there are and, when the window does not hold the graph, an arc whose
// span exceeds W / 2 - 64; begin() allocates (E_NOMEM naming the back-pointer bytes) and sets alpha to -inf, batch() takes the
// log-prob rows of the next frames (one encoded batch), advance() runs the kernel over the frames of the batch whose rows lie in the
// slab (slabs in row order), finish() back-traces: states as CtcGraphAligner's, score, and the path's smallest distance in nodes to
// a window edge that is not the graph's own.
enum { CTC_GRAPH_WINDOW_MAX_NODES = 8192, CTC_GRAPH_WINDOW_DEFAULT_NODES = 8192 };
struct CtcGraphWindowTables {
  int N = 0, startmax = -1;                        // nodes; the highest node with a start predecessor
  std::vector<int32_t> M;                          // [N]: the largest successor of any node <= j (j itself where there is none)
  std::vector<int32_t> E;                          // E[r]: the lowest node from which a final one is at most r frames away (r beyond: E.back())
};
struct CtcGraphWindowStep { int lo, f1; };
// the launch that starts at frame f0 of a slab that ends at fend: its window and its end, given the window before and the node of the
// first-maximum state of the last frame (-1: none finite).  1. lo = 0 at frame 0, else centred on the best node, never back, never
// past the graph's end; 2. f1 = the frame before which the climber (M applied once a frame) would leave through the window's top, at
// least f0 + 1, at most fend; 3. lo raised until the window's last node is at least E[T - f1]
CtcGraphWindowStep ctc_graph_window_next(const CtcGraphWindowTables& g, int T, int W, int f0, int fend, int lo_prev, int best_prev);
struct CtcGraphWindowAligner {
  int N = 0, T = 0, W = 0, blank = 0;
  bool has_wild = false, open = false;
  float bias = 0.f;
  CtcGraphWindowTables tab;
  std::vector<int32_t> h_tokens, h_arc_off, h_finals, h_rows;   // h_rows: the rows of the batch being fed, its first frame is lattice frame fbase
  std::vector<uint32_t> h_arcs;                    // per arc: the span j - p (start: j + 1) | (first arc: the node has a start arc) << 29 | last of its list << 30 | allow-T << 31
  int fed = 0, fbase = 0;                          // lattice frames advanced so far
  int lo = 0, best = -1, launches = 0;             // the last launch's window and the best node it reported
  const int32_t* lo_force = nullptr;               // lab hook: every slab is ONE launch, in the window lo_force[launch]
  int n_force = 0;
  size_t bp_bytes = 0;
  DevBuf d_tokens, d_arc_off, d_arcs, d_finals, d_rows, d_alpha, d_bp, d_lo, d_best, d_states, d_end;
  int plan(const char* who, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final,
           int64_t total_frames, int window_nodes, int V, int blank_id, float wildcard_bias);
  int begin(hipStream_t s);
  int batch(hipStream_t s, const std::vector<int32_t>& rows);
  bool touches(int r0, int nrows) const;
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax = nullptr);
  int finish(hipStream_t s, int32_t* states /* [T]: 2 * slot + token bit */, float* score, int32_t* min_margin, int32_t* lo_out = nullptr /* [T] */);
  void release();
};

// ---- long-form full-sum scoring over a token graph (ctc_graph_fb_window.hip): CtcGraphScorer's two sweeps inside
// CtcGraphWindowAligner's moving window, shared by rvb_ctc_score_graph_long_* and the lab hook.  plan() makes
// CtcGraphWindowAligner::plan's checks in its words with this lattice's window cap (the fp64 states halve it), refuses wildcards and,
// with posteriors, an out-degree above the in-degree cap, and builds the live-set words and the transposed arcs (no device work);
// begin() allocates (with posteriors: T x W x 4 bytes of alpha rows, or E_NOMEM naming them); batch() / advance() feed the encoded
// batches in ascending order, the launches cut by ctc_graph_window_next from the best node each launch reports (the host keeps every
// launch's frames, window and best node); loglik() ends the forward sweep; batch_back() / advance_back() take the same batches in
// DESCENDING order, slabs descending within a batch, and replay the recorded launches in reverse; finish() returns the per-node
// reductions.
enum { CTC_GRAPH_SCORE_WINDOW_MAX_NODES = 4096, CTC_GRAPH_SCORE_WINDOW_DEFAULT_NODES = 4096 };
struct CtcGraphWindowScorer {
  struct Launch { int f0, f1, lo, best; };
  int N = 0, T = 0, W = 0, blank = 0;
  bool open = false, post = false, forward_done = false;
  CtcGraphWindowTables tab;
  std::vector<int32_t> h_tokens, h_arc_off, h_finals, h_rows, h_succ_off;   // h_rows: the rows of the batch being fed, its first frame is lattice frame fbase
  std::vector<uint32_t> h_arcs;                    // CtcGraphWindowAligner's words
  std::vector<uint32_t> h_succs;                   // per successor: the span j' - j | last of its list << 30 | T_j' may be entered from T_j << 31
  std::vector<uint32_t> h_rem;                     // per node: the fewest frames from T_j, from B_j to a final end; then B_start's
  std::vector<uint8_t> h_fin;
  std::vector<Launch> launches;                    // the forward launches in order: they tile [0, fed)
  std::vector<int> batches;                        // frames of every forward batch, in order
  int fed = 0, fbase = 0;                          // forward: lattice frames advanced so far
  int lo = 0, best = -1;                           // the last launch's window and the best node it reported
  int back = 0, back_batch = 0, cursor = 0;        // backward: frames still to go, batches still to come, launches below the cursor
  const int32_t* lo_force = nullptr;               // lab hook: every slab is ONE launch, in the window lo_force[launch]
  int n_force = 0;
  size_t row_bytes = 0;
  DevBuf d_tokens, d_arc_off, d_arcs, d_finals, d_rows, d_rem, d_alpha, d_lo, d_csum, d_loglik, d_llhat, d_best, d_coff, d_arows, d_beta,
      d_acc, d_succ_off, d_succs, d_fin;
  int plan(const char* who, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final,
           int64_t total_frames, int window_nodes, int V, int blank_id, bool posteriors);
  int begin(hipStream_t s);
  int batch(hipStream_t s, const std::vector<int32_t>& rows);
  bool touches(int r0, int nrows) const;
  int advance(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int loglik(hipStream_t s, double* loglik_out);
  int batch_back(hipStream_t s, const std::vector<int32_t>& rows);
  int advance_back(hipStream_t s, const float* lp, int ld, int r0, int nrows);
  int finish(hipStream_t s, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame /* per node, nullable */);
  void release();
};

}  // namespace rvb

struct rvb_engine {
  rvb_model_cfg cfg;
  int device = 0;
  int dtype = 0;
  bool fp8 = false;              // RVB_FP8: dtype stays DT_BF16, the encoder's feed-forward / qkv / pointwise GEMMs run in fp8
  int f8_state = 0;              // 0 not calibrated, 1 calibrating (bf16 pass collecting max |.|), 2 fp8 GEMMs active
  std::vector<rvb::F8Scales> f8;
  std::vector<unsigned> f8_groups;   // per block: which GEMM groups run in fp8 (bit 0 ffm, 1 qkv, 2 pw1, 3 pw2, 4 ff)
  rvb::DevBuf d_amax;            // fp32 [blocks + 1][8]; row `blocks`, slot 0: the subsampling's conv1 output (conv2's fp8 operand)
  bool f8_conv2 = false;         // policy bit 5: conv2 of the subsampling (K = 9 d, 27 % of the encoder's FLOPs) in fp8
  float f8_x1 = 0.f;             // calibrated scale of conv1's output (0: not calibrated -> conv2 stays bf16)
  rvb::DevBuf d_f8sat;           // uint32 [blocks + 1][8]: values clipped at +-448 per activation slot (rvb_get_fp8_saturation)
  hipStream_t stream = nullptr;
  bool finalized = false;

  std::map<std::string, rvb::HostTensor> host;   // staged state dict (fp32)

  // ---- packed weights ----
  rvb::DevBuf cmvn_mean, cmvn_istd, conv1_w, conv1_b;
  rvb::Linear conv2, embed_out, ctc;
  rvb::LNorm enc_after;
  std::vector<rvb::EncLayer> enc;
  rvb::Decoder dec_l, dec_r;
  rvb::DevBuf pe_f32;            // fp32 [pe_rows][d] sinusoid table
  int pe_rows = 0;
  rvb::DevBuf fb_window, fb_twiddle, fb_melw, fb_lo, fb_hi;
  rvb::DevBuf stage;             // fp32 staging for weight packing

  // ---- audio / features ----
  rvb::DevBuf pcm, feats;        // int16 [n], fp32 [chunks*T0pad][80]
  // double-buffered upload (rvb_upload_pcm_async): the NEXT recording's samples travel on `copy_stream` into `pcm_next` while
  // the current one is being decoded; the next rvb_fbank waits for `pcm_ready` on the engine's stream and swaps the buffers
  rvb::DevBuf pcm_next;
  hipStream_t copy_stream = nullptr;
  hipEvent_t pcm_ready = nullptr, pcm_free = nullptr;   // pcm_free: the last fbank that read `pcm` has run
  bool pcm_pending = false;
  int64_t n_samples_next = 0;
  rvb::DevBuf wave_f32, rs_kernel; // the waveform the fbank reads when it is not int16 PCM at 16 kHz: resampled and / or uploaded as float
  rvb::DevBuf wave_in;             // a float waveform at another rate, before resampling (rvb_upload_wave_f32)
  bool pcm_is_float = false;
  int dec_chunk = 0, dec_left = -1;   // encoder chunk mask (decoding_chunk_size / num_decoding_left_chunks), 0 = full context
  int64_t n_samples = 0, n_frames = 0, feat_rows = 0;
  // rvb_upload_batch: several recordings resident together.  16 kHz int16 recordings are packed in `pcm`, float ones and the
  // resampler's outputs in `wave_f32` (resampler inputs: `pcm` / `wave_in`); a single upload clears `batch` and vice versa
  bool batch = false;
  std::vector<int64_t> batch_n, batch_src;       // per recording: 16 kHz samples; element offset in the buffer the fbank reads
  std::vector<int32_t> batch_is_float;
  std::vector<int64_t> h_frame0;                 // host images of the descriptors of the last rvb_fbank_batch
  std::vector<rvb::FbankRec> h_rec;
  rvb::DevBuf d_frame0, d_rec;
  // rvb_pause_chunks (pause_chunks.hip): `feats` keeps the frame-ordered rows; while `packed` is set rvb_encode reads the pieces from
  // `feats_packed` instead (packed_rows rows).  Every upload and every fbank call clears `packed`.
  int feat_kind = 0;                             // what `feats` holds: 0 nothing, 1 rvb_fbank's rows, 2 rvb_fbank_batch's
  bool packed = false;
  int64_t packed_rows = 0;
  rvb::DevBuf feats_packed, pc_loud, pc_rec, pc_frame0, pc_table, pc_count, pc_pieces;

  // ---- batch state ----
  int B = 0, T0 = 0, T1 = 0, F1 = 0, T2 = 0, F2 = 0, beam = 0;
  std::vector<int32_t> in_lens, enc_lens;
  rvb::DevBuf d_feats_in, X1, X2, x, xn, y, h, ao, dconv, enc_out, logits, topv, topi;
  rvb::DevBuf d_enc_lens, d_seq_start, d_seq_len, d_aux_i32;
  float* h_topv = nullptr;         // pinned host copies of the per-frame top-k (async D2H per slice)
  int32_t* h_topi = nullptr;
  size_t h_top_cap = 0;
  struct Slice { int c0, nb; hipEvent_t ev; bool done; };
  std::vector<Slice> slices;       // slices of the last rvb_encode, in chunk order
  std::vector<hipEvent_t> slice_event_pool;
  int xattn_max_rows = 0;          // most decoder rows of any chunk (cross-attention query sequence length)
  const int* cur_lens = nullptr;   // device pointer: valid encoder frames of the slice being encoded
  std::vector<rvb::PrefixResult> nbest;
  std::shared_ptr<const rvb::ContextGraph> context_graph;   // rvb_set_context_graph: biases every later rvb_ctc_prefix_beam (null: none)
  std::vector<rvb::RescoreResult> rescored;
  std::vector<rvb::TrieBatch> trie_l;   // per chunk, local numbering: built by the prefix-beam workers for the rescoring decoder
  rvb::HostPool pool;                   // host workers of the CTC search and the trie building
  std::vector<rvb::JointResult> joint;           // rvb_joint_decode: winner per chunk
  std::vector<rvb::DevBuf> jkv;                   // joint_decoding: per decoder layer T [rows][2d], key | value of every decoded prefix
  rvb::DevBuf jlogp, jpair_row, jpair_tok, jpair_out;     // fp32 [rows][V] log-softmax after each decoded prefix; pair gather buffers
  int64_t joint_rows = 0, joint_steps = 0;       // decoder rows computed / batched decoder steps of the last rvb_joint_decode
  float last_blank_penalty = 0.f;                // of the last rvb_encode / rvb_stream_finish
  std::vector<std::vector<int>> attn_tokens;     // rvb_attention_decode: best hypothesis per chunk
  std::vector<float> attn_scores;
  rvb::DevBuf atopv, atopi;                       // per-step top-k of the decoder output
  std::vector<rvb::DevBuf> kcache, vcache, kcache2, vcache2, memkv;   // per decoder layer
  // decoder workspace
  rvb::DevBuf dx, dxn, dy, dh, dqkv, dq, dao, kvmem, d_tok, d_pos, d_tgt, d_logp;
  rvb::DevBuf d_hq_start, d_hq_len, d_hkv_start, d_hkv_len;
  rvb::DevBuf d_hq_pos0, d_hpath_start, d_hpath_len, d_path, d_work, d_tgt_ptr;    // rescoring over the hypothesis trie
  int64_t rescore_rows = 0, rescore_pairs = 0;      // decoder rows computed / (hypothesis, position) pairs served, last call
  rvb::DevBuf d_xlse, d_xsum, d_xtop;               // rvb_attention_score: lse fp32, sum of logits fp64, arg-max int32 per trie row

  // ---- streaming encoder (forward_chunk with caches, encoder.py:231-402) ----
  struct StreamState {
    bool active = false;
    int offset = 0;                 // encoder frames produced so far (`offset` of forward_chunk)
    int cache_len = 0;              // frames in the attention cache (cache_t1)
    std::vector<rvb::DevBuf> kv, kv2;   // per layer T [pe_rows][2d]: key | value rows of the cached frames (+ spare for trimming)
    int cnn_rows = 0;               // real frames in the cnn cache (cache_t2 grows to lorder = K-1; older = zero padding)
    std::vector<rvb::DevBuf> cnn, cnn2; // causal conv module, per layer T [K-1][2d]: pointwise-conv1 outputs of the last frames
  } stream_st;
  rvb::DevBuf d_stream_i32;         // {kv_start = 0, kv_len = cache + chunk}

  // ---- encoder taps (rvb_set_encoder_tap / rvb_get_encoder_tap: read-only, for the tests' stage-by-stage check) ----
  int tap_block = -1;               // -1 off; 0 .. blocks - 1: that conformer block; blocks: the front end before block 0
  bool tap_live = false;            // rvb_encode is inside the tapped position: tap_keep() copies, tap_note_gemm() notes
  struct Tap { rvb::DevBuf buf; size_t elems = 0; bool bf16 = false; };
  std::map<std::string, Tap> taps;  // what the last tapped rvb_encode kept, by name (device copies, made on the engine's stream)
  std::vector<float> tap_forms;     // the forms that ran there: see rvb_get_encoder_tap "forms"
  // decoder taps (rvb_set_decoder_tap / rvb_get_decoder_tap): the same tap_keep() / tap_note_gemm(); a tapped decoder_forward swaps
  // these in for `taps` / `tap_forms` while it runs, so the encoder's kept copies and the decoder's never mix
  int dtap_side = 0, dtap_pos = -1; // side 0 left / 1 right; position -1 off, 0 .. layers - 1 a layer, layers the head
  int dtap_rows = 0;                // trie rows of the last tapped run
  std::map<std::string, Tap> dtaps;
  std::vector<float> dtap_forms, dtap_trie;   // forms as above (+ attention_last_form's eight per attention); the trie's host arrays

  // ---- forced alignment (rvb_ctc_align) ----
  rvb::CtcAligner aligner;
  rvb::CtcScorer scorer;           // rvb_ctc_score
  rvb::CtcFinder finder;           // rvb_ctc_find
  rvb::CtcGraphAligner graph_aligner;   // rvb_ctc_align_graph
  rvb::CtcGraphScorer graph_scorer;     // rvb_ctc_score_graph
  rvb::CtcWindowAligner long_aligner;   // rvb_ctc_align_long_*: its own member, so the calls above stay usable between begin and finish
  rvb::CtcWindowScorer long_scorer;     // rvb_ctc_score_long_*: likewise
  rvb::CtcGraphWindowAligner long_graph_aligner;   // rvb_ctc_align_graph_long_*: likewise
  rvb::CtcGraphWindowScorer long_graph_scorer;     // rvb_ctc_score_graph_long_*: likewise
  rvb::DevBuf align_lp, align_tv, align_ti, align_row, align_col, align_out;   // fp32 [LOGIT_SLAB][V] log-softmax slab; gather scratch

  // ---- RCCL communicator of the C-ABI collectives (comm.hip; optional) ----
  void* comm = nullptr;
  int comm_world = 1, comm_rank = 0;
  rvb::DevBuf comm_send, comm_recv;

  // ---- profiling ----
  int profiling = 0;     // 0 off, 1 every stage, 2 GEMM launches only (what the roofline needs; half the events)
  std::map<std::string, rvb::ProfEntry> prof;
  struct Pending { hipEvent_t a, b; std::string name; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
};
