// CTC forced alignment of a known transcript (the reference's force_align, asr/wenet/utils/ctc_utils.py:105-161, called from
// bin/alignment.py:233-242): Viterbi over the extended sequence z = [b, y0, b, y1, ..., y(L-1), b], S = 2L + 1 states.
//
//   alpha[0][0] = lp[0][z0], alpha[0][1] = lp[0][z1], -inf elsewhere
//   alpha[t][s] = max(alpha[t-1][s], alpha[t-1][s-1] (, alpha[t-1][s-2] if z[s] != b, s >= 2, z[s] != z[s-2])) + lp[t][z[s]]
//   back-pointer = the FIRST maximum in the order s, s-1, s-2; end = the better of states S-1 and S-2, S-1 on a tie.
//
// The only arithmetic is one fp32 addition per cell (no multiply, so nothing to contract) and comparisons: with the same lp bits
// the result equals a host evaluation of the same recurrence label for label, ties included.
//
// Shape: ONE workgroup per lattice, no cooperation between workgroups.  Each thread owns SPT consecutive states in registers
// (SPT = 4 / 16 / 32, up to 1024 threads: S <= 32 768); the only value that crosses threads is the last alpha of the left
// neighbour, through a double-buffered LDS array: one __syncthreads() per frame.  The emissions lp[t+1][z[s]] of the NEXT frame
// are gathered from the [rows, V] log-softmax slab before the barrier of frame t (and the slab row of frame t+2 is read then), so no
// memory latency sits between two barriers.  Back-pointers are 2 bits per cell in HBM (a thread's SPT states = one 1 / 4 / 8 byte store
// per frame); alpha lives in HBM between launches, so the pass advances slab by slab as the engine produces the log-probs.
// The back-trace is one lane walking T dependent 1-byte loads.  Every loop is bounded by T or SPT.
//
// Wildcards (WILD = true; dispatched only when a sequence of the call holds one): a transcript position with the id
// RVB_CTC_WILDCARD is an ordinary token state (stay / from its blank / from two below when that token is another label; two
// adjacent wildcards are the same label) whose emission at frame t is ew = w[row] + bias, w = the row's maximum over all V columns,
// one fp32 addition.  A per-thread bit mask marks the owned wildcards; ew is one more workgroup-uniform value per frame, loaded
// with eb from a [rows] array beside the slab and double-buffered with it, and a wildcard takes it in place of its gathered
// column (whose load, of the blank's column, stays in bounds and is discarded).  The select sits where et[k] is consumed, not
// where it is refilled: ew then travels exactly as eb does and no step waits for a load it issued itself.  Barriers, LDS,
// back-pointers and the back-trace are those of the plain form.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rvb {

namespace {

template <int SPT> struct BpWord;
template <> struct BpWord<4> { typedef uint8_t type; };
template <> struct BpWord<16> { typedef uint32_t type; };
template <> struct BpWord<32> { typedef unsigned long long type; };

template <int SPT, bool WILD>
__global__ __launch_bounds__(1024) void ctc_viterbi_forward_kernel(const VitSeq* __restrict__ seqs, const float* __restrict__ lp, int ld,
                                                                   int r0, const int* __restrict__ rows, const int* __restrict__ tokens,
                                                                   int blank, float* __restrict__ alpha_all, uint8_t* __restrict__ bp_all,
                                                                   const float* __restrict__ wmax, float bias) {
  constexpr int NT = SPT / 2;                      // tokens per thread: local state 2k + 1 is token s0 / 2 + k, even states are blank
  typedef typename BpWord<SPT>::type word_t;
  __shared__ float bnd[2][1024];                   // per thread: alpha of its last state (all a right neighbour reads: its first state is a
                                                   // blank, which has no s-2 predecessor)
  const VitSeq q = seqs[blockIdx.x];
  if (q.f0 >= q.f1) return;                        // nothing of this lattice in the slab (uniform over the workgroup)
  const int tid = threadIdx.x;
  const int s0 = tid * SPT;
  const int S = q.S;
  const float NEG = -INFINITY;
  const int nvalid = min(max(S - s0, 0), SPT);     // states of this thread that exist
  const int* y = tokens + q.tok_off;
  const int* rw = rows + q.frame_off;
  float* alpha = alpha_all + q.alpha_off;
  word_t* bp = (word_t*)(bp_all + q.bp_off) + tid;
  const size_t bp_stride = (size_t)q.bp_stride / sizeof(word_t);

  unsigned tok[NT];                                // byte offset of each token's column in a row of lp (32 bits: uniform row base + lane offset)
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
      tok[k] = (unsigned)((WILD && id == RVB_CTC_WILDCARD) ? blank : id) * 4u;   // the wildcard's gather: a column that exists
    }
  }

  float a[SPT];
  // Emissions of two frames in registers (A: frames f, f + 2, ...; B: the frames between).  A frame's step consumes one buffer and
  // refills each register right after its use with the emission two frames on: loads stay in flight across two barriers and
  // nothing is copied.  Rows past the last frame of this launch are clamped to it (a harmless in-bounds load).
  float ebA, etA[NT], ebB, etB[NT];
  float ewA = 0.f, ewB = 0.f;                      // WILD: the wildcard's emission of the frame, buffered with eb
  int f = q.f0;
  auto row_of = [&](int fr) { return rw[min(fr, q.f1 - 1)] - r0; };
  auto fill = [&](float& eb, float& ew, float* et, int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
    if (WILD) ew = wmax[r] + bias;
#pragma unroll
    for (int k = 0; k < NT; ++k) et[k] = *(const float*)(row + tok[k]);
  };
  constexpr bool TWO = SPT < 32;                   // 32 states per thread: one buffer (refilled one frame ahead) is what fits 128 VGPRs
  constexpr int D = TWO ? 2 : 1;                   // frames between a register's use and the use of its refill
  fill(ebA, ewA, etA, row_of(f));
  if (TWO) fill(ebB, ewB, etB, row_of(f + 1));
  int rA = row_of(f + D), rB = row_of(f + D + 1);  // the rows the next refill of A / B reads, fetched ahead of their use
  int par = 0;

  auto step = [&](float& eb, float& ew, float* et, int fr, int refill_row) {
    const char* row = (const char*)(lp + (size_t)refill_row * ld);
    const float left = tid > 0 ? bnd[par][tid - 1] : NEG;
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
        // states past S - 1 hold junk that no real state reads (predecessors lie below)
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
    par ^= 1;
    bnd[par][tid] = a[SPT - 1];
    __syncthreads();
  };

  if (f == 0) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = NEG;
    if (tid == 0) { a[0] = ebA; a[1] = (WILD && (wild & 1u)) ? ewA : etA[0]; }
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
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < nvalid) alpha[s0 + j] = a[j];
}

// one lane per lattice: end state, then T - 1 dependent back-pointer loads
__global__ void ctc_viterbi_backtrace_kernel(const VitSeq* __restrict__ seqs, const float* __restrict__ alpha_all,
                                             const uint8_t* __restrict__ bp_all, int* __restrict__ states, float* __restrict__ score) {
  if (threadIdx.x != 0) return;
  const VitSeq q = seqs[blockIdx.x];
  const float* alpha = alpha_all + q.alpha_off;
  const uint8_t* bp = bp_all + q.bp_off;
  int* out = states + q.frame_off;
  const float a1 = alpha[q.S - 1], a2 = alpha[q.S - 2];
  int st = a2 > a1 ? q.S - 2 : q.S - 1;
  score[blockIdx.x] = a2 > a1 ? a2 : a1;
  for (int t = q.T - 1; t >= 1; --t) {
    out[t] = st;
    const unsigned code = (bp[(size_t)t * q.bp_stride + (st >> 2)] >> ((st & 3) * 2)) & 3u;
    st = max(st - (int)code, 0);
  }
  out[0] = st;
}

}  // namespace

int ctc_viterbi_forward(hipStream_t s, const VitSeq* seqs, int n_seq, int max_S, const float* lp, int ld, int r0, const int* rows,
                        const int* tokens, int blank, float* alpha, uint8_t* bp, const float* wmax, float bias) {
  if (n_seq <= 0) return OK;
  if (max_S < 3 || max_S > CTC_ALIGN_MAX_STATES) { set_error("ctc_viterbi_forward: states out of range"); return E_ARG; }
  const int spt = ctc_spt_for(max_S), threads = ctc_threads(max_S, spt);
#define RVB_VIT_(SPT, WILD) ctc_viterbi_forward_kernel<SPT, WILD><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, alpha, bp, wmax, bias)
  if (wmax) {                                      // some sequence of the call holds a wildcard
    if (spt == 4) RVB_VIT_(4, true);
    else if (spt == 16) RVB_VIT_(16, true);
    else RVB_VIT_(32, true);
  } else {
    if (spt == 4) RVB_VIT_(4, false);
    else if (spt == 16) RVB_VIT_(16, false);
    else RVB_VIT_(32, false);
  }
#undef RVB_VIT_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int ctc_viterbi_backtrace(hipStream_t s, const VitSeq* seqs, int n_seq, const float* alpha, const uint8_t* bp, int* states, float* score) {
  if (n_seq <= 0) return OK;
  ctc_viterbi_backtrace_kernel<<<n_seq, 64, 0, s>>>(seqs, alpha, bp, states, score);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcAligner::plan(const char* who, const int32_t* tokens, const int32_t* tok_lens, int n_seq,
                     const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id, bool allow_wild) {
  const std::string w(who);
  if (!tokens || !tok_lens || n_seq <= 0 || (int)seq_rows.size() != n_seq) { set_error(w + ": null argument or no sequence"); return E_ARG; }
  if (V < 2 || blank_id < 0 || blank_id >= V) { set_error(w + ": blank id outside [0, V)"); return E_ARG; }
  seq.assign(n_seq, VitSeq{});
  h_tokens.clear(); h_rows.clear();
  max_S = 0; blank = blank_id; has_wild = false;
  size_t alpha_off = 0, bp_off = 0;
  int64_t tok_off = 0, frame_off = 0;
  for (int i = 0; i < n_seq; ++i) {
    const int L = tok_lens[i];
    const int64_t T = (int64_t)seq_rows[i].size();
    const std::string at = w + ": sequence " + std::to_string(i) + ": ";
    if (L <= 0) { set_error(at + "empty transcript (L = 0): nothing to align"); return E_ARG; }
    if (L > CTC_ALIGN_MAX_TOKENS) {
      set_error(at + std::to_string(L) + " tokens exceed the cap of " + std::to_string(CTC_ALIGN_MAX_TOKENS) + " tokens (" +
                std::to_string(CTC_ALIGN_MAX_STATES) + " states) per lattice");
      return E_UNSUPPORTED;
    }
    RVB_TRY(slab_frame_cap(at, T, CTC_ALIGN_MAX_FRAMES, "lattice"));
    const int32_t* y = tokens + tok_off;
    int repeats = 0;
    for (int k = 0; k < L; ++k) {
      if (allow_wild && y[k] == RVB_CTC_WILDCARD) { has_wild = true; if (k && y[k - 1] == y[k]) ++repeats; continue; }
      if (y[k] < 0 || y[k] >= V) { set_error(at + "token id " + std::to_string(y[k]) + " outside [0, " + std::to_string(V) + ")"); return E_ARG; }
      if (y[k] == blank_id) { set_error(at + "token " + std::to_string(k) + " is the blank id " + std::to_string(blank_id)); return E_ARG; }
      if (k && y[k] == y[k - 1]) ++repeats;
    }
    if (T < (int64_t)L + repeats) {
      set_error(at + "infeasible: " + std::to_string(L) + " tokens with " + std::to_string(repeats) + " adjacent repeats need at least " +
                std::to_string(L + repeats) + " frames, the lattice has " + std::to_string(T));
      return E_ARG;
    }
    VitSeq& q = seq[i];
    q.L = L; q.S = 2 * L + 1; q.T = (int)T;
    q.tok_off = (int)tok_off; q.frame_off = (int)frame_off;
    const int spt_unit = 32;                                  // layout independent of the instantiation chosen for the batch
    const size_t s_pad = (size_t)(q.S + spt_unit - 1) / spt_unit * spt_unit;
    q.alpha_off = (long long)alpha_off; q.bp_off = (long long)bp_off; q.bp_stride = (long long)(s_pad / 4);
    alpha_off += s_pad;
    bp_off += (size_t)T * (s_pad / 4);
    max_S = std::max(max_S, q.S);
    h_tokens.insert(h_tokens.end(), y, y + L);
    tok_off += L;
    RVB_TRY(slab_take_rows(w, at, seq_rows[i], &h_rows, &frame_off));
  }
  alpha_floats = alpha_off; bp_bytes = bp_off; total_frames = frame_off;
  return OK;
}

int CtcAligner::begin(hipStream_t s) {
  RVB_TRY(d_tokens.ensure(h_tokens.size() * 4));
  RVB_TRY(d_rows.ensure(h_rows.size() * 4));
  RVB_TRY(d_seqs.ensure(seq.size() * sizeof(VitSeq)));
  RVB_TRY(d_alpha.ensure(alpha_floats * 4));
  RVB_TRY(d_states.ensure((size_t)total_frames * 4));
  RVB_TRY(d_score.ensure(seq.size() * 4));
  if (int r = d_bp.ensure(bp_bytes)) {
    set_error("ctc align: " + std::to_string(bp_bytes) + " bytes of back-pointers (2 bits per frame and state) do not fit: " + last_error());
    return r;
  }
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), h_tokens.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice, s));
  for (auto& q : seq) q.f0 = q.f1 = 0;
  return OK;
}

int CtcAligner::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax, float bias) {
  if (has_wild && !wmax) { set_error("ctc align: a transcript with wildcards needs the row maxima"); return E_ARG; }
  bool any;
  RVB_TRY(slab_window("ctc align", false, seq, h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, d_seqs.p, seq));
  return ctc_viterbi_forward(s, d_seqs.as<VitSeq>(), (int)seq.size(), max_S, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), blank,
                             d_alpha.as<float>(), d_bp.as<uint8_t>(), has_wild ? wmax : nullptr, bias);
}

int CtcAligner::finish(hipStream_t s, int32_t* states, float* score) {
  RVB_TRY(slab_covered("ctc align", false, seq));
  RVB_TRY(ctc_viterbi_backtrace(s, d_seqs.as<VitSeq>(), (int)seq.size(), d_alpha.as<float>(), d_bp.as<uint8_t>(), d_states.as<int>(),
                                 d_score.as<float>()));
  RVB_HIP_CHECK(hipMemcpyAsync(states, d_states.p, (size_t)total_frames * 4, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipMemcpyAsync(score, d_score.p, seq.size() * 4, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  return slab_feasible("ctc align", seq, score, "emits the transcript");
}

void CtcAligner::release() {
  for (DevBuf* b : {&d_tokens, &d_rows, &d_seqs, &d_alpha, &d_bp, &d_states, &d_score}) b->release();
}

}  // namespace rvb
