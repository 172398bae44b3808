// CTC phrase search: every occurrence of short token phrases in the log-probs of a recording ("where are these terms spoken?").
//
// A phrase y[0..L-1], 1 <= L <= 32, is the lattice z = [y0, b, y1, b, ..., y(L-1)] of S = 2L - 1 <= 63 states, WITHOUT a leading or
// trailing blank: an occurrence starts on its first token and ends on its last.  With w[t] = the maximum of row t of lp over all V
// columns (what a wildcard frame of ctc_viterbi.hip emits) the emission is d[t][s] = lp[t][z[s]] - w[t] <= 0, one fp32 subtraction,
// and the path score one fp32 addition per cell (nothing to contract):
//
//   h[-1][.] = -inf
//   h[t][0]  = max(h[t-1][0], 0) + d[t][0]                       the 0: "the occurrence starts at frame t"
//   h[t][s]  = max(h[t-1][s], h[t-1][s-1] (, h[t-1][s-2] if z[s] is a token, s >= 2, z[s] != z[s-2])) + d[t][s]
//   st[t][s] = the start frame of the chosen predecessor, t for a fresh start; the FIRST maximum in the order stay, one below
//              (state 0: the fresh start), two below, which is the aligner's order
//
// Frame t is an ARRIVAL if the chosen predecessor of state S - 1 is not "stay"; as every d <= 0, staying on the last token never
// raises a score, so the best end of any path is its arrival and only arrivals can be hits.  An arrival with h[t][S-1] >= the
// phrase's threshold is a CANDIDATE (end = t, start = st[t][S-1], score = h[t][S-1]); the host suppresses overlapping ones.
//
// Shape: ONE WAVE per (phrase, sequence) pair, FIND_WAVES pairs per workgroup; waves share nothing, so there is no LDS and no
// barrier, and a wave whose pair does not exist (or has no frame in the slab) returns at once.  Lane s owns state s; lane 63 and the
// lanes at or above S compute values nobody reads.  h and st of the two lower neighbours come by __shfl_up (ds_bpermute_b32: four
// independent cross-lane moves per frame, issued back to back, so their latencies overlap).  The serial chain of a frame is
// therefore: the cross-lane moves, two compares with their selects, one add.  (A DPP wave_shr:1 move would shorten the chain; it
// waits for a run on the device that shows what it gains -- docs/tuning-log.md section 14.)
//
// Emissions: lane s gathers column z[s] of the row; w comes from the row-maximum array the log-softmax kernel fills.  The loads of
// frame t + FIND_AHEAD are issued before frame t is computed (a ring of FIND_AHEAD registers, the loop unrolled by the same number,
// so nothing is copied); the row index each load needs is fetched a further FIND_AHEAD frames ahead, so no load waits for another.
// FIND_AHEAD = 8: one frame of the chain is about 80 - 100 cycles, a load that misses L2 and hits the Infinity Cache about 550 (the
// slab was written by the kernel before this one, 8192 rows x V x 4 bytes, more than L2 holds): 8 frames cover it, and 2 x 8 + 8
// registers are nothing.  Rows past the last frame of the launch are clamped to it (an in-bounds load that is discarded).
//
// The pass advances slab by slab like CtcAligner::advance; h and st (64 floats + 64 ints per pair) and the candidate count live in
// HBM between launches, so the result does not depend on where the slabs are cut.  Candidates are written by the lane of state
// S - 1 into the pair's own buffer in frame order with plain vector stores -- no atomics; the count is a register of that lane.  The
// first max_candidates are kept, every one is counted.  Every loop is bounded by the slab's frame count.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

namespace rvb {

namespace {

constexpr int FIND_WAVES = 4;                      // pairs per workgroup
constexpr int FIND_AHEAD = 8;                      // frames between a load and its use

// lane i receives lane i - 1's value; lane 0 keeps its own (which the caller replaces)
__device__ __forceinline__ float up1(float v) { return __shfl_up(v, 1); }
__device__ __forceinline__ int up1(int v) { return __shfl_up(v, 1); }

__global__ __launch_bounds__(FIND_WAVES * 64) void ctc_find_kernel(const FindSeq* __restrict__ seqs, const FindPhrase* __restrict__ phrases,
                                                                   int n_seq, int n_pairs, const float* __restrict__ lp, int ld, int r0,
                                                                   const int* __restrict__ rows, const int* __restrict__ tokens,
                                                                   int blank, const float* __restrict__ wmax, float* __restrict__ h_all,
                                                                   int* __restrict__ st_all, long long* __restrict__ count_all,
                                                                   int max_cand, int* __restrict__ cand_end, int* __restrict__ cand_start,
                                                                   float* __restrict__ cand_score) {
  // the wave's pair, in a scalar register: descriptors, row indices, row maxima and loop bounds are then scalar too
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.x * FIND_WAVES + (threadIdx.x >> 6));
  if (pair >= n_pairs) return;
  const FindSeq q = seqs[pair % n_seq];
  if (q.f0 >= q.f1) return;                        // nothing of this sequence in the slab
  const FindPhrase ph = phrases[pair / n_seq];
  const int lane = threadIdx.x & 63;
  const int S = 2 * ph.L - 1;
  const int* y = tokens + ph.tok_off;
  const int* rw = rows + q.frame_off;
  const float NEG = -INFINITY;

  // the lanes at or above S read the blank's column (a column that exists) and never skip
  const bool tok_state = lane < S && !(lane & 1);
  const int zid = tok_state ? y[lane >> 1] : blank;
  const bool skip = tok_state && lane >= 2 && zid != y[(lane >> 1) - 1];
  const unsigned col = (unsigned)zid * 4u;
  const bool last = lane == S - 1;

  float h;
  int st;
  long long count = 0;
  const size_t slot = (size_t)pair * 64 + lane;
  if (q.f0 == 0) { h = NEG; st = 0; }
  else { h = h_all[slot]; st = st_all[slot]; if (last) count = count_all[pair]; }
  int* ce = cand_end + (size_t)pair * max_cand;
  int* cs = cand_start + (size_t)pair * max_cand;
  float* cv = cand_score + (size_t)pair * max_cand;

  auto row_of = [&](int fr) { return rw[min(fr, q.f1 - 1)] - r0; };
  float e[FIND_AHEAD], wv[FIND_AHEAD];             // lp[t][z] and w[t] of the frames f .. f + FIND_AHEAD - 1
  int rr[FIND_AHEAD];                              // the rows of the frames f + FIND_AHEAD .. f + 2 FIND_AHEAD - 1
#pragma unroll
  for (int k = 0; k < FIND_AHEAD; ++k) {
    const int r = row_of(q.f0 + k);
    e[k] = *(const float*)((const char*)(lp + (size_t)r * ld) + col);
    wv[k] = wmax[r];
    rr[k] = row_of(q.f0 + FIND_AHEAD + k);
  }

  for (int f = q.f0; f < q.f1; f += FIND_AHEAD) {
#pragma unroll
    for (int k = 0; k < FIND_AHEAD; ++k) {
      const int t = f + k;
      if (t < q.f1) {                              // wave-uniform
        const float d = e[k] - wv[k];
        float c1 = up1(h);
        int s1 = up1(st);
        const float c2 = __shfl_up(h, 2);          // lanes 0 and 1 never use it (skip is false there)
        const int s2 = __shfl_up(st, 2);
        if (lane == 0) { c1 = 0.f; s1 = t; }       // the fresh start
        float best = h;
        int from = st;
        bool moved = false;
        if (c1 > best) { best = c1; from = s1; moved = true; }
        if (skip && c2 > best) { best = c2; from = s2; moved = true; }
        h = best + d;
        st = from;
        if (last && moved && h >= ph.threshold) {
          if (count < max_cand) { ce[count] = t; cs[count] = from; cv[count] = h; }
          ++count;
        }
      }
      // refill: frame t + FIND_AHEAD from the row fetched a round ago, then the row of frame t + 2 FIND_AHEAD
      e[k] = *(const float*)((const char*)(lp + (size_t)rr[k] * ld) + col);
      wv[k] = wmax[rr[k]];
      rr[k] = row_of(t + 2 * FIND_AHEAD);
    }
  }
  h_all[slot] = h;
  st_all[slot] = st;
  if (last) count_all[pair] = count;
}

}  // namespace

int ctc_find_advance(hipStream_t s, const FindSeq* seqs, const FindPhrase* phrases, int n_seq, int n_phrases, const float* lp, int ld,
                     int r0, const int* rows, const int* tokens, int blank, const float* wmax, float* h, int* st, long long* count,
                     int max_cand, int* cand_end, int* cand_start, float* cand_score) {
  const long long n_pairs = (long long)n_seq * n_phrases;
  if (n_pairs <= 0) return OK;
  if (n_pairs > std::numeric_limits<int>::max() / 64 || max_cand < 1) { set_error("ctc_find_advance: pairs or cap out of range"); return E_ARG; }
  const int blocks = (int)((n_pairs + FIND_WAVES - 1) / FIND_WAVES);
  ctc_find_kernel<<<blocks, FIND_WAVES * 64, 0, s>>>(seqs, phrases, n_seq, (int)n_pairs, lp, ld, r0, rows, tokens, blank, wmax, h, st, count,
                                                     max_cand, cand_end, cand_start, cand_score);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcFinder::plan(const char* who, const int32_t* tokens, const int32_t* tok_lens, int n_phr, const float* threshold,
                    const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id, int max_candidates) {
  const std::string w(who);
  const int n_seq = (int)seq_rows.size();
  if (!tokens || !tok_lens || !threshold) { set_error(w + ": null argument"); return E_ARG; }
  if (n_phr < 1 || n_seq < 1) { set_error(w + ": need n_phrases >= 1 and n_seq >= 1"); return E_ARG; }
  if (max_candidates < 1) { set_error(w + ": need max_candidates >= 1"); return E_ARG; }
  if (V < 2 || blank_id < 0 || blank_id >= V) { set_error(w + ": blank id outside [0, V)"); return E_ARG; }
  phr.assign(n_phr, FindPhrase{});
  seq.assign(n_seq, FindSeq{});
  h_tokens.clear(); h_rows.clear();
  blank = blank_id; max_cand = max_candidates;
  int64_t tok_off = 0, frame_off = 0;
  for (int p = 0; p < n_phr; ++p) {
    const int L = tok_lens[p];
    const std::string at = w + ": phrase " + std::to_string(p) + ": ";
    if (L <= 0) { set_error(at + "empty phrase (L = 0): nothing to find"); return E_ARG; }
    if (L > CTC_FIND_MAX_TOKENS) {
      set_error(at + std::to_string(L) + " tokens exceed the cap of " + std::to_string(CTC_FIND_MAX_TOKENS) +
                " tokens per phrase (one wave holds the lattice); a longer text is located by rvb_ctc_align_wild with a wildcard on either side");
      return E_UNSUPPORTED;
    }
    const int32_t* y = tokens + tok_off;
    for (int k = 0; k < L; ++k) {
      if (y[k] < 0 || y[k] >= V) { set_error(at + "token id " + std::to_string(y[k]) + " outside [0, " + std::to_string(V) + ")"); return E_ARG; }
      if (y[k] == blank_id) { set_error(at + "token " + std::to_string(k) + " is the blank id " + std::to_string(blank_id)); return E_ARG; }
    }
    if (!(threshold[p] <= 0.f)) {                  // NaN fails the comparison too
      set_error(at + "threshold must be <= 0 (total nats; -inf keeps every arrival) and not NaN");
      return E_ARG;
    }
    phr[p].tok_off = (int)tok_off; phr[p].L = L; phr[p].threshold = threshold[p];
    h_tokens.insert(h_tokens.end(), y, y + L);
    tok_off += L;
  }
  for (int i = 0; i < n_seq; ++i) {
    const int64_t T = (int64_t)seq_rows[i].size();
    const std::string at = w + ": sequence " + std::to_string(i) + ": ";
    RVB_TRY(slab_frame_cap(at, T, CTC_ALIGN_MAX_FRAMES, "sequence"));
    seq[i].frame_off = (int)frame_off; seq[i].T = (int)T;
    RVB_TRY(slab_take_rows(w, at, seq_rows[i], &h_rows, &frame_off));
  }
  const double pairs = (double)n_phr * n_seq;
  const double bytes = pairs * max_candidates * 12.0;
  if (pairs > (double)(std::numeric_limits<int>::max() / 64) || bytes > CTC_FIND_MAX_CANDIDATE_BYTES) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.0f", bytes);
    set_error(w + ": " + buf + " bytes of candidate buffers (" + std::to_string(n_phr) + " phrases x " + std::to_string(n_seq) +
              " sequences x " + std::to_string(max_candidates) + " candidates x 12 bytes) do not fit: ask with a smaller max_candidates");
    return E_NOMEM;
  }
  return OK;
}

int CtcFinder::begin(hipStream_t s) {
  const size_t pairs = phr.size() * seq.size();
  RVB_TRY(d_tokens.ensure(h_tokens.size() * 4));
  RVB_TRY(d_rows.ensure(h_rows.size() * 4));
  RVB_TRY(d_seqs.ensure(seq.size() * sizeof(FindSeq)));
  RVB_TRY(d_phr.ensure(phr.size() * sizeof(FindPhrase)));
  RVB_TRY(d_h.ensure(pairs * 64 * 4));
  RVB_TRY(d_st.ensure(pairs * 64 * 4));
  RVB_TRY(d_count.ensure(pairs * 8));
  const size_t cand = pairs * (size_t)max_cand;
  for (DevBuf* b : {&d_cend, &d_cstart, &d_cscore})
    if (int r = b->ensure(cand * 4)) {
      set_error("ctc find: " + std::to_string(cand * 12) + " bytes of candidate buffers (12 bytes per pair and candidate) do not fit: " + last_error());
      return r;
    }
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), h_tokens.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_phr.p, phr.data(), phr.size() * sizeof(FindPhrase), hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemsetAsync(d_count.p, 0, pairs * 8, s));     // a sequence without frames never runs the kernel
  for (auto& q : seq) q.f0 = q.f1 = 0;
  return OK;
}

int CtcFinder::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax) {
  if (!lp || !wmax) { set_error("ctc find: the slab and its row maxima are needed"); return E_ARG; }
  bool any;
  RVB_TRY(slab_window("ctc find", false, seq, h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, d_seqs.p, seq));
  return ctc_find_advance(s, d_seqs.as<FindSeq>(), d_phr.as<FindPhrase>(), (int)seq.size(), (int)phr.size(), lp, ld, r0, d_rows.as<int>(),
                          d_tokens.as<int>(), blank, wmax, d_h.as<float>(), d_st.as<int>(), d_count.as<long long>(), max_cand,
                          d_cend.as<int>(), d_cstart.as<int>(), d_cscore.as<float>());
}

// Non-maximum suppression within one pair: by score descending, then end ascending, then start ascending; a candidate is kept if
// [start, end] meets no kept span; the max_hits best are kept and returned in order of end.
int ctc_find_suppress(const int32_t* end, const int32_t* start, const float* score, int n, int max_hits, int32_t* out_start,
                      int32_t* out_end, float* out_score) {
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    if (score[a] != score[b]) return score[a] > score[b];
    if (end[a] != end[b]) return end[a] < end[b];
    return start[a] < start[b];
  });
  std::vector<int> kept;
  for (int i : order) {
    if ((int)kept.size() >= max_hits) break;
    bool clear = true;
    for (int k : kept)
      if (start[i] <= end[k] && start[k] <= end[i]) { clear = false; break; }
    if (clear) kept.push_back(i);
  }
  std::sort(kept.begin(), kept.end(), [&](int a, int b) { return end[a] < end[b]; });    // kept spans are disjoint: ends differ
  for (size_t k = 0; k < kept.size(); ++k) { out_start[k] = start[kept[k]]; out_end[k] = end[kept[k]]; out_score[k] = score[kept[k]]; }
  return (int)kept.size();
}

int CtcFinder::finish(hipStream_t s, int max_hits, int32_t* n_hits, int32_t* start, int32_t* end, float* score, int64_t* n_candidates,
                      int32_t* raw_end, int32_t* raw_start, float* raw_score) {
  RVB_TRY(slab_covered("ctc find", false, seq));
  const size_t pairs = phr.size() * seq.size();
  std::vector<long long> count(pairs);
  RVB_HIP_CHECK(hipMemcpyAsync(count.data(), d_count.p, pairs * 8, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  // the kept candidates of every pair, packed: the whole buffers in three copies while they are small, else pair by pair
  std::vector<size_t> off(pairs + 1, 0);
  for (size_t p = 0; p < pairs; ++p) off[p + 1] = off[p] + (size_t)std::min<long long>(count[p], max_cand);
  const size_t total = pairs * (size_t)max_cand;
  const bool whole = total <= ((size_t)4 << 20);
  const size_t n_host = whole ? total : off[pairs];
  std::vector<int32_t> ce(n_host), cs(n_host);
  std::vector<float> cv(n_host);
  if (whole) {
    RVB_HIP_CHECK(hipMemcpyAsync(ce.data(), d_cend.p, total * 4, hipMemcpyDeviceToHost, s));
    RVB_HIP_CHECK(hipMemcpyAsync(cs.data(), d_cstart.p, total * 4, hipMemcpyDeviceToHost, s));
    RVB_HIP_CHECK(hipMemcpyAsync(cv.data(), d_cscore.p, total * 4, hipMemcpyDeviceToHost, s));
  } else {
    for (size_t p = 0; p < pairs; ++p) {
      const size_t kept = off[p + 1] - off[p];
      if (!kept) continue;
      RVB_HIP_CHECK(hipMemcpyAsync(ce.data() + off[p], d_cend.as<int>() + p * max_cand, kept * 4, hipMemcpyDeviceToHost, s));
      RVB_HIP_CHECK(hipMemcpyAsync(cs.data() + off[p], d_cstart.as<int>() + p * max_cand, kept * 4, hipMemcpyDeviceToHost, s));
      RVB_HIP_CHECK(hipMemcpyAsync(cv.data() + off[p], d_cscore.as<float>() + p * max_cand, kept * 4, hipMemcpyDeviceToHost, s));
    }
  }
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  std::vector<int32_t> hs((size_t)max_hits), he((size_t)max_hits);
  std::vector<float> hv((size_t)max_hits);
  // results are assembled first and handed over whole, so a failure above leaves the caller's arrays as they were
  std::vector<int32_t> o_n(pairs), o_s(pairs * max_hits), o_e(pairs * max_hits);
  std::vector<float> o_v(pairs * max_hits);
  for (size_t p = 0; p < pairs; ++p) {
    const int kept = (int)(off[p + 1] - off[p]);
    const size_t at = whole ? p * max_cand : off[p];
    if (raw_end) std::copy(ce.begin() + at, ce.begin() + at + kept, raw_end + p * max_cand);
    if (raw_start) std::copy(cs.begin() + at, cs.begin() + at + kept, raw_start + p * max_cand);
    if (raw_score) std::copy(cv.begin() + at, cv.begin() + at + kept, raw_score + p * max_cand);
    const int n = ctc_find_suppress(ce.data() + at, cs.data() + at, cv.data() + at, kept, max_hits, hs.data(), he.data(), hv.data());
    o_n[p] = n;
    std::copy(hs.begin(), hs.begin() + n, o_s.begin() + p * max_hits);
    std::copy(he.begin(), he.begin() + n, o_e.begin() + p * max_hits);
    std::copy(hv.begin(), hv.begin() + n, o_v.begin() + p * max_hits);
  }
  for (size_t p = 0; p < pairs; ++p) {
    n_hits[p] = o_n[p];
    std::copy(o_s.begin() + p * max_hits, o_s.begin() + p * max_hits + o_n[p], start + p * max_hits);
    std::copy(o_e.begin() + p * max_hits, o_e.begin() + p * max_hits + o_n[p], end + p * max_hits);
    std::copy(o_v.begin() + p * max_hits, o_v.begin() + p * max_hits + o_n[p], score + p * max_hits);
    if (n_candidates) n_candidates[p] = count[p];
  }
  return OK;
}

void CtcFinder::release() {
  for (DevBuf* b : {&d_tokens, &d_rows, &d_seqs, &d_phr, &d_h, &d_st, &d_count, &d_cend, &d_cstart, &d_cscore}) b->release();
}

}  // namespace rvb
