// Windowed CTC Viterbi: forced alignment of a transcript of any length over a lattice that arrives in several encoded batches.
//
// The recurrence, the order of the predecessors (s, s-1, s-2), the first-maximum rule and the end rule are those of ctc_viterbi.hip.
// What differs: at every frame only W consecutive states of z = [b, y0, b, ..., y(L-1), b] are alive, the window [lo, lo + W).
// A state outside the window is -inf: the left neighbour of the window's first state is -inf, and nothing is written above its last.
// lo is a multiple of 32, never decreases and changes only BETWEEN launches (it is a field of the launch's descriptor), so inside a
// launch the kernel is the plain one shifted by lo: thread tid owns the states lo + tid * SPT ..., an even state is a blank, and a
// thread's back-pointer word sits at the same place of the frame's row whatever lo is.
//
//   alpha        fp32 [S_pad], the WHOLE lattice, -inf at begin(); a launch reads its window's states and writes them back.  A state
//                above every window so far still holds -inf, one below lo is never read again.
//   back-ptrs    2 bits per cell, window-relative: T x W / 4 bytes (not T x S / 4); lo_of[t] (int32 per frame, a plain vector
//                store of thread 0) tells the back-trace where frame t's row starts.
//   best         after its last frame the workgroup reduces the alpha of its window to the FIRST maximum (the lowest state on a
//                tie; -1 when every state is -inf): 8 bytes the host reads back to place the next window (ctc_window_next_lo).
//
// One workgroup, no cooperation with any other; one LDS exchange and one __syncthreads() per frame; emissions gathered one or two
// frames ahead; every loop bounded by T, SPT or W.  With W >= S the window never moves and the result is ctc_viterbi.hip's bit for
// bit; otherwise it is the best path among those that stay inside the windows, and the back-trace reports how close that path
// came to a window edge that is not the lattice's own edge.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rvb {

namespace {

template <int SPT> struct WinWord;
template <> struct WinWord<4> { typedef uint8_t type; };
template <> struct WinWord<16> { typedef uint32_t type; };
template <> struct WinWord<32> { typedef unsigned long long type; };

struct WinSeg {            // one launch: the lattice, its window and the frames to advance over
  int L, S, T, W;          // tokens, states 2 L + 1, frames of the whole lattice, states of the window (a multiple of 32)
  int lo;                  // first state of the window (a multiple of 32; 0 in the launch that holds frame 0)
  int f0, f1;              // lattice frames this launch advances (f0 == 0: initialise; else continue from alpha in HBM)
  int fbase;               // the lattice frame of rows[0]: frame f reads row rows[f - fbase] - r0 of lp
};
struct WinBest { int state; float value; };
struct WinEnd { float score; int margin; int clamped; int pad_; };

template <int SPT, bool WILD>
__global__ __launch_bounds__(1024) void ctc_viterbi_window_kernel(const WinSeg q, const float* __restrict__ lp, int ld, int r0,
                                                                  const int* __restrict__ rows, const int* __restrict__ y, int blank,
                                                                  float* __restrict__ alpha, uint8_t* __restrict__ bp_all,
                                                                  int* __restrict__ lo_of, WinBest* __restrict__ best_out,
                                                                  const float* __restrict__ wmax, float bias) {
  constexpr int NT = SPT / 2;                      // tokens per thread: local state 2k + 1 is token s0 / 2 + k, even states are blank
  typedef typename WinWord<SPT>::type word_t;
  __shared__ float bnd[2][1024];                   // per thread: alpha of its last state, all its right neighbour reads
  __shared__ float red_v[16];
  __shared__ int red_s[16];
  if (q.f0 >= q.f1) return;                        // uniform over the workgroup
  const int tid = threadIdx.x;
  const int s0 = q.lo + tid * SPT;                 // first state of this thread in the lattice
  const int S = q.S;
  const float NEG = -INFINITY;
  const bool mine = tid * SPT < q.W;               // the launch rounds the threads up to whole waves: some own nothing
  const int nvalid = mine ? min(max(S - s0, 0), SPT) : 0;     // states of this thread that exist
  word_t* bp = (word_t*)bp_all + tid;
  const size_t bp_stride = (size_t)(q.W / 4) / sizeof(word_t);

  unsigned tok[NT];                                // byte offset of each token's column in a row of lp
  unsigned skip = 0;                               // bit k: state 2k + 1 may be entered from two states below
  unsigned wild = 0;                               // bit k: token k is a wildcard (WILD only)
  {
    int prev = (s0 >= 2 && s0 / 2 - 1 < q.L) ? y[s0 / 2 - 1] : -1;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int i = s0 / 2 + k;
      const bool have = i < q.L;
      const int id = have ? y[i] : blank;          // a column that exists, for the states past S - 1
      if (have && i >= 1 && id != prev) skip |= 1u << k;
      prev = id;
      if (WILD && id == RVB_CTC_WILDCARD) wild |= 1u << k;
      tok[k] = (unsigned)((WILD && id == RVB_CTC_WILDCARD) ? blank : id) * 4u;
    }
  }

  float a[SPT];
  float ebA, etA[NT], ebB, etB[NT];                // emissions of two frames in registers, as in ctc_viterbi.hip
  float ewA = 0.f, ewB = 0.f;
  int f = q.f0;
  auto row_of = [&](int fr) { return rows[min(fr, q.f1 - 1) - q.fbase] - r0; };
  auto fill = [&](float& eb, float& ew, float* et, int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
    if (WILD) ew = wmax[r] + bias;
#pragma unroll
    for (int k = 0; k < NT; ++k) et[k] = *(const float*)(row + tok[k]);
  };
  constexpr bool TWO = SPT < 32;                   // 32 states per thread: one buffer (refilled one frame ahead) is what fits 128 VGPRs
  constexpr int D = TWO ? 2 : 1;
  fill(ebA, ewA, etA, row_of(f));
  if (TWO) fill(ebB, ewB, etB, row_of(f + 1));
  int rA = row_of(f + D), rB = row_of(f + D + 1);
  int par = 0;

  auto step = [&](float& eb, float& ew, float* et, int fr, int refill_row) {
    const char* row = (const char*)(lp + (size_t)refill_row * ld);
    const float left = tid > 0 ? bnd[par][tid - 1] : NEG;     // below the window: -inf
    word_t codes = 0;
#pragma unroll
    for (int j = SPT - 1; j >= 0; --j) {           // downwards: a[j-1], a[j-2] still hold frame fr - 1
      const float c1 = j >= 1 ? a[j - 1] : left;
      float best = a[j];
      unsigned code = 0;
      if (c1 > best) { best = c1; code = 1; }
      if (j & 1) {
        const float c2 = j >= 2 ? a[j - 2] : left;
        if (((skip >> (j >> 1)) & 1u) && c2 > best) { best = c2; code = 2; }
        if (WILD) a[j] = best + (((wild >> (j >> 1)) & 1u) ? ew : et[j >> 1]);
        else a[j] = best + et[j >> 1];
        et[j >> 1] = *(const float*)(row + tok[j >> 1]);
      } else {
        a[j] = best + eb;
      }
      codes |= (word_t)code << (2 * j);
    }
    eb = *(const float*)(row + (unsigned)blank * 4u);
    if (WILD) ew = wmax[refill_row] + bias;
    if (nvalid > 0) bp[(size_t)fr * bp_stride] = codes;
    if (tid == 0) lo_of[fr] = q.lo;
    par ^= 1;
    bnd[par][tid] = a[SPT - 1];
    __syncthreads();
  };

  if (f == 0) {                                    // the window of frame 0 starts at state 0
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = NEG;
    if (tid == 0) { a[0] = ebA; a[1] = (WILD && (wild & 1u)) ? ewA : etA[0]; lo_of[0] = q.lo; }
    fill(ebA, ewA, etA, rA);
    rA = row_of(f + 2 * D);
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = j < nvalid ? alpha[s0 + j] : NEG;
  }
  bnd[0][tid] = a[SPT - 1];
  __syncthreads();
  if (TWO) {
    if (f == 0) {
      f = 1;
      if (f < q.f1) { step(ebB, ewB, etB, f, rB); rB = row_of(f + 4); ++f; }
    }
    for (; f + 1 < q.f1; f += 2) {
      step(ebA, ewA, etA, f, rA);
      rA = row_of(f + 4);
      step(ebB, ewB, etB, f + 1, rB);
      rB = row_of(f + 5);
    }
    if (f < q.f1) step(ebA, ewA, etA, f, rA);
  } else {
    if (f == 0) f = 1;
    for (; f < q.f1; ++f) {
      step(ebA, ewA, etA, f, rA);
      rA = row_of(f + 2);
    }
  }
  float bv = NEG;                                  // the first maximum of the window: lowest state on a tie, -1 when all are -inf
  int bs = -1;
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < nvalid) {
      alpha[s0 + j] = a[j];
      if (a[j] > bv) { bv = a[j]; bs = s0 + j; }
    }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64);
    const int s2 = __shfl_xor(bs, o, 64);
    if (v2 > bv || (v2 == bv && (unsigned)s2 < (unsigned)bs)) { bv = v2; bs = s2; }
  }
  if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_s[tid >> 6] = bs; }
  __syncthreads();
  if (tid == 0) {
    const int nw = (int)blockDim.x >> 6;
    for (int w = 1; w < nw; ++w)
      if (red_v[w] > bv || (red_v[w] == bv && (unsigned)red_s[w] < (unsigned)bs)) { bv = red_v[w]; bs = red_s[w]; }
    best_out->state = bs;
    best_out->value = bv;
  }
}

// one lane: end state, then T - 1 dependent back-pointer loads, each in the row of its own frame's window
__global__ void ctc_viterbi_window_backtrace_kernel(int S, int T, int W, const float* __restrict__ alpha, const uint8_t* __restrict__ bp,
                                                    const int* __restrict__ lo_of, int* __restrict__ states, WinEnd* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int S_pad = (S + 31) / 32 * 32;
  const size_t stride = (size_t)(W / 4);
  const float a1 = alpha[S - 1], a2 = alpha[S - 2];
  int st = a2 > a1 ? S - 2 : S - 1;
  int margin = W, clamped = 0;
  for (int t = T - 1; t >= 0; --t) {
    const int lo = lo_of[t];
    states[t] = st;
    int idx = st - lo;
    if (idx < 0 || idx >= W) { clamped = 1; idx = min(max(idx, 0), W - 1); }      // cannot happen on a path with a finite score
    if (lo != 0) margin = min(margin, idx);                                      // the lattice's own edges do not count
    if (lo + W < S_pad) margin = min(margin, W - 1 - idx);
    if (t == 0) break;
    const unsigned code = (bp[(size_t)t * stride + (idx >> 2)] >> ((idx & 3) * 2)) & 3u;
    st = max(st - (int)code, 0);
  }
  out->score = a2 > a1 ? a2 : a1;
  out->margin = margin;
  out->clamped = clamped;
}

int window_forward(hipStream_t s, const WinSeg& q, const float* lp, int ld, int r0, const int* rows, const int* tokens, int blank,
                   float* alpha, uint8_t* bp, int* lo_of, WinBest* best, const float* wmax, float bias) {
  const int spt = ctc_spt_for(q.W), threads = ctc_threads(q.W, spt);
#define RVB_WIN_(SPT, WILD) \
  ctc_viterbi_window_kernel<SPT, WILD><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, alpha, bp, lo_of, best, wmax, bias)
  if (wmax) {
    if (spt == 4) RVB_WIN_(4, true);
    else if (spt == 16) RVB_WIN_(16, true);
    else RVB_WIN_(32, true);
  } else {
    if (spt == 4) RVB_WIN_(4, false);
    else if (spt == 16) RVB_WIN_(16, false);
    else RVB_WIN_(32, false);
  }
#undef RVB_WIN_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int round_down32(int v) { return v >= 0 ? v / 32 * 32 : -((-v + 31) / 32 * 32); }

}  // namespace

// ------------------------------------------------------------------------------------ the window policy (host only, pure)
int ctc_window_next_lo(int S, int T, int W, int f0, int f1, int lo_prev, int best_prev) {
  const int S_pad = (S + 31) / 32 * 32;
  if (f0 <= 0) return 0;                                                  // the first launch: frame 0 lives in states 0 and 1
  int lo = best_prev >= 0 ? round_down32(best_prev - W / 2) : lo_prev;    // 1. centre on the best state (none finite: stay)
  lo = std::max(lo, lo_prev);                                             // 2. never back
  lo = std::min(lo, round_down32(2 * f0 + 1));                            // 3. not above the highest state frame f0 can reach,
  lo = std::min(lo, S_pad - W);                                           //    nor past the lattice's end
  const int need = S - 2 - 2 * (T - f1);                                  // 4. at frame f1 - 1 the window still holds a state from
  if (lo + W - 1 < need) lo = (need - W + 1 + 31) / 32 * 32;              //    which S - 2 is reachable in the frames that remain
  return std::max(lo, lo_prev);                                           // a state below lo is never read again: never back
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcWindowAligner::plan(const char* who, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states, int V,
                           int blank_id, bool allow_wild, float wildcard_bias) {
  const std::string w(who), at = w + ": ";
  if (!tokens) { set_error(w + ": null argument"); return E_ARG; }
  if (V < 2 || blank_id < 0 || blank_id >= V) { set_error(w + ": blank id outside [0, V)"); return E_ARG; }
  if (!(std::isfinite(wildcard_bias) && wildcard_bias <= 0.f)) { set_error(w + ": wildcard_bias must be finite and <= 0"); return E_ARG; }
  if (window_states != 0 && (window_states < 256 || window_states > CTC_WINDOW_MAX_STATES || window_states % 256 != 0)) {
    set_error(at + "window_states " + std::to_string(window_states) + " must be 0 (the default, " + std::to_string(CTC_WINDOW_DEFAULT_STATES) +
              ") or a multiple of 256 in [256, " + std::to_string(CTC_WINDOW_MAX_STATES) + "]");
    return E_ARG;
  }
  if (n_tokens <= 0) { set_error(at + "empty transcript (L = 0): nothing to align"); return E_ARG; }
  if (total_frames < 1) { set_error(at + "need total_frames >= 1"); return E_ARG; }
  RVB_TRY(slab_frame_cap(at, total_frames, CTC_ALIGN_MAX_FRAMES, "lattice"));
  bool wild_seen = false;
  int64_t repeats = 0;
  for (int k = 0; k < n_tokens; ++k) {
    if (allow_wild && tokens[k] == RVB_CTC_WILDCARD) { wild_seen = true; if (k && tokens[k - 1] == tokens[k]) ++repeats; continue; }
    if (tokens[k] < 0 || tokens[k] >= V) { set_error(at + "token id " + std::to_string(tokens[k]) + " outside [0, " + std::to_string(V) + ")"); return E_ARG; }
    if (tokens[k] == blank_id) { set_error(at + "token " + std::to_string(k) + " is the blank id " + std::to_string(blank_id)); return E_ARG; }
    if (k && tokens[k] == tokens[k - 1]) ++repeats;
  }
  if (total_frames < (int64_t)n_tokens + repeats) {
    set_error(at + "infeasible: " + std::to_string(n_tokens) + " tokens with " + std::to_string(repeats) + " adjacent repeats need at least " +
              std::to_string((int64_t)n_tokens + repeats) + " frames, the lattice has " + std::to_string(total_frames));
    return E_ARG;
  }
  L = n_tokens; S = 2 * L + 1; S_pad = (S + 31) / 32 * 32; T = (int)total_frames;
  W = std::min(window_states ? window_states : (int)CTC_WINDOW_DEFAULT_STATES, S_pad);
  blank = blank_id; has_wild = wild_seen; bias = wildcard_bias;
  bp_bytes = (size_t)T * (size_t)(W / 4);
  h_tokens.assign(tokens, tokens + L);
  h_rows.clear();
  fed = fbase = 0; lo = 0; best = -1; open = false;
  return OK;
}

int CtcWindowAligner::begin(hipStream_t s) {
  RVB_TRY(d_tokens.ensure((size_t)L * 4));
  RVB_TRY(d_alpha.ensure((size_t)S_pad * 4));
  RVB_TRY(d_lo.ensure((size_t)T * 4));
  RVB_TRY(d_states.ensure((size_t)T * 4));
  RVB_TRY(d_best.ensure(sizeof(WinBest)));
  RVB_TRY(d_end.ensure(sizeof(WinEnd)));
  if (int r = d_bp.ensure(bp_bytes)) {
    set_error("ctc align long: " + std::to_string(bp_bytes) + " bytes of back-pointers (2 bits per frame and window state) do not fit: " + last_error());
    return r;
  }
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
  const float ninf = -INFINITY;
  int bits;
  memcpy(&bits, &ninf, 4);
  RVB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_alpha.p, bits, (size_t)S_pad, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));          // h_tokens may be replaced by the next plan()
  open = true;
  return OK;
}

int CtcWindowAligner::batch(hipStream_t s, const std::vector<int32_t>& rows) {
  if (!open) { set_error("ctc align long: feed before begin"); return E_STATE; }
  if (fed != fbase + (int64_t)h_rows.size()) { set_error("ctc align long: the slabs did not cover every frame of the batch before"); return E_STATE; }
  if (fed + (int64_t)rows.size() > T) {
    set_error("ctc align long: feed after the lattice's frames are used up: " + std::to_string(fed) + " of " + std::to_string(T) +
              " frames fed, the batch holds " + std::to_string(rows.size()) + " more");
    return E_STATE;
  }
  for (size_t f = 1; f < rows.size(); ++f)
    if (rows[f] <= rows[f - 1]) { set_error("ctc align long: frame rows must increase"); return E_ARG; }
  h_rows = rows;
  fbase = fed;
  RVB_TRY(d_rows.ensure(std::max<size_t>(rows.size(), 1) * 4));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  RVB_HIP_CHECK(hipMemcpy(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice));
  return OK;
}

bool CtcWindowAligner::touches(int r0, int nrows) const {
  const auto a = std::lower_bound(h_rows.begin(), h_rows.end(), r0), b = std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows);
  return a != b;
}

int CtcWindowAligner::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax) {
  if (!open) { set_error("ctc align long: feed before begin"); return E_STATE; }
  if (has_wild && !wmax) { set_error("ctc align long: a transcript with wildcards needs the row maxima"); return E_ARG; }
  const int b0 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0) - h_rows.begin());
  const int b1 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows) - h_rows.begin());
  if (b0 == b1) return OK;
  if (fbase + b0 != fed) { set_error("ctc align long: slabs must arrive in row order"); return E_STATE; }
  // A path climbs at most 2 states a frame, and centring rounds lo down by up to 31 states: W / 4 - 16 frames climb W / 2 - 32, so a
  // path at the window's centre cannot leave through the top within one launch.  A window below 160 states never moves (W = S_pad).
  const int seg = W / 4 > 32 ? W / 4 - 16 : std::max(W / 4, 1);
  for (int g0 = fbase + b0, end = fbase + b1; g0 < end; g0 += seg) {
    const int g1 = std::min(g0 + seg, end);
    lo = ctc_window_next_lo(S, T, W, g0, g1, lo, best);
    WinSeg q{L, S, T, W, lo, g0, g1, (int)fbase};
    RVB_TRY(window_forward(s, q, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), blank, d_alpha.as<float>(), d_bp.as<uint8_t>(),
                           d_lo.as<int>(), d_best.as<WinBest>(), has_wild ? wmax : nullptr, bias));
    WinBest hb;
    RVB_HIP_CHECK(hipMemcpyAsync(&hb, d_best.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    RVB_HIP_CHECK(hipStreamSynchronize(s));        // the one synchronisation of a launch: the next window depends on it
    best = hb.state;
    fed = g1;
  }
  return OK;
}

int CtcWindowAligner::finish(hipStream_t s, int32_t* states, float* score, int32_t* min_margin, int32_t* lo_out) {
  if (!open) { set_error("ctc align long: finish before begin"); return E_STATE; }
  if (fed != T) {
    set_error("ctc align long: finish before all " + std::to_string(T) + " frames were fed (" + std::to_string(fed) + " so far)");
    return E_STATE;
  }
  ctc_viterbi_window_backtrace_kernel<<<1, 64, 0, s>>>(S, T, W, d_alpha.as<float>(), d_bp.as<uint8_t>(), d_lo.as<int>(), d_states.as<int>(),
                                                       d_end.as<WinEnd>());
  RVB_HIP_CHECK(hipGetLastError());
  WinEnd he;
  std::vector<int32_t> st((size_t)T), lo_host(lo_out ? (size_t)T : 0);
  RVB_HIP_CHECK(hipMemcpyAsync(st.data(), d_states.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  if (lo_out) RVB_HIP_CHECK(hipMemcpyAsync(lo_host.data(), d_lo.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipMemcpyAsync(&he, d_end.p, sizeof(he), hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  if (!(he.score > -INFINITY)) {
    set_error("ctc align long: infeasible: no path inside the window of " + std::to_string(W) + " states emits the transcript over " +
              std::to_string(T) + " frames with a finite score");
    return E_ARG;
  }
  if (he.clamped) { set_error("ctc align long: the back-trace left its window on a path with a finite score"); return E_HIP; }
  memcpy(states, st.data(), (size_t)T * 4);        // nothing is written before the last check: a refusal leaves the outputs untouched
  if (lo_out) memcpy(lo_out, lo_host.data(), (size_t)T * 4);
  if (score) *score = he.score;
  if (min_margin) *min_margin = he.margin;
  return OK;
}

void CtcWindowAligner::release() {
  for (DevBuf* b : {&d_tokens, &d_rows, &d_alpha, &d_bp, &d_lo, &d_best, &d_states, &d_end}) b->release();
  open = false;
}

}  // namespace rvb
