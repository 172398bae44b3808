// CTC forced alignment over a left-to-right token GRAPH (alternatives and optional words): the Viterbi pass of ctc_viterbi.hip with
// arbitrary earlier nodes as predecessors.  A graph has N token nodes in topological order; node j has a label tok[j] (a vocab id or
// RVB_CTC_WILDCARD), an ordered predecessor list pred[j][0..d) of earlier nodes or -1 ("start"), and a final flag.  States: B_start
// (the leading blank) and per node T_j (emits its label) and B_j (the blank after it).
//
//   frame 0:  B_start = lp[0][blank];  T_j = emission if -1 is in pred[j], else -inf;  B_j = -inf
//   frame t:  B_start: stay.   B_j: stay, then T_j.
//             T_j: stay, then for k = 0..d-1: B_{pred k} (B_start for -1), then T_{pred k} if pred k is a node of another label
//             the FIRST maximum wins (strict >), new value = winner + emission (one fp32 addition)
//   end:      over the final nodes in ascending order: B_f, then T_f, first maximum.
//
// On a chain (pred[j] = [j-1], pred[0] = [-1], last node final) this is the recurrence of ctc_viterbi.hip candidate for candidate
// (s, s-1, s-2 = stay, the blank before, the token before), so labels and score have the same bits.
//
// Shape: ONE workgroup per lattice, one __syncthreads() per frame.  Thread tid owns nodes tid, tid + nthreads, ... (NPT = 1 / 2 / 4 / 8
// of them, up to 1024 threads: N <= 8192) with their T and B in registers.  Every node PUBLISHES its pair {T, B} of the frame in a
// double-buffered LDS array (slot 0 = {-inf, B_start}, slot j + 1 = node j; 2 x 8193 x 8 bytes = 128 KiB at the cap, of the 160 KiB
// one workgroup may hold), and a predecessor is one 8-byte LDS read: with the interleaved ownership the lanes of a wave read
// consecutive slots on a chain, which is conflict-free.  An arc is one 32-bit word, slot | allow-T << 15, laid out by the host; the
// first arc of each owned node lives in a register, so a node of in-degree 1 (every node of a chain, most nodes of a transcript)
// touches no memory but LDS; the further arcs are read from HBM through the L1 each frame.  The emissions of the NEXT frame are
// gathered before the barrier of frame t, as in the chain kernel.
//
// Back-pointers are ONE byte per node and frame: bits 0-6 = T_j's winner (0 stay, 1 + k = predecessor k; in-degree <= 64), bit 7 =
// B_j's winner (1 = from T_j).  Which of B_p / T_p a predecessor p contributed is not stored: the two are adjacent candidates, so T_p
// won over B_p exactly when T_p(t-1) > B_p(t-1), and that comparison IS bit 7 of p's byte of the same frame.  The layout (bytes per
// frame = N padded to 64) does not depend on the instantiation.  alpha ({T, B} per slot) lives in HBM between launches, so the pass
// advances slab by slab.  The back-trace is one lane walking T dependent loads (two per frame when it follows an arc).  Every loop
// is bounded by T, a node count or an in-degree.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace rvb {

namespace {

template <int NPT>
__global__ __launch_bounds__(1024) void ctc_graph_forward_kernel(const GraphSeq* __restrict__ seqs, const float* __restrict__ lp, int ld,
                                                                 int r0, const int* __restrict__ rows, const int* __restrict__ node_tok,
                                                                 const int* __restrict__ arc_off_all, const unsigned* __restrict__ arcs_all,
                                                                 int blank, float* __restrict__ alpha_all, uint8_t* __restrict__ bp_all,
                                                                 const float* __restrict__ wmax, float bias, int slots_cap) {
  extern __shared__ __attribute__((aligned(16))) char cg_smem[];
  float2* pub = (float2*)cg_smem;                  // [2][slots_cap]: {T, B} of every slot, frames t - 1 and t
  const GraphSeq q = seqs[blockIdx.x];
  if (q.f0 >= q.f1) return;                        // nothing of this lattice in the slab (uniform over the workgroup)
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = q.N;
  const float NEG = -INFINITY;
  const int* rw = rows + q.frame_off;
  const int* aoff = arc_off_all + q.node_off + q.index;        // N + 1 offsets per lattice
  const unsigned* arcs = arcs_all + q.arc_off;
  float2* alpha = (float2*)(alpha_all + q.alpha_off);           // [N + 1] slots
  uint8_t* bp = bp_all + q.bp_off;

  unsigned col[NPT];                               // byte offset of the node's column in a row of lp (the blank's for a wildcard)
  unsigned arc0[NPT];                              // the node's first arc
  unsigned meta[NPT];                              // where its further arcs start | its in-degree << 16 (0: no such node)
  unsigned wild = 0;                               // bit k: owned node k is a wildcard
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = tid + k * nth;
    col[k] = (unsigned)blank * 4u; arc0[k] = 0; meta[k] = 0;
    if (j < N) {
      const int id = node_tok[q.node_off + j];
      if (id == RVB_CTC_WILDCARD) wild |= 1u << k; else col[k] = (unsigned)id * 4u;
      const int o = aoff[j];
      meta[k] = (unsigned)(o + 1) | (unsigned)(aoff[j + 1] - o) << 16; arc0[k] = arcs[o];
    }
  }

  auto row_of = [&](int fr) { return rw[min(fr, q.f1 - 1)] - r0; };   // past the launch's last frame: clamped, a harmless in-bounds load
  float eb, ew = 0.f, et[NPT];
  auto fill = [&](float& b, float& w, float* e, int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    b = *(const float*)(row + (unsigned)blank * 4u);
    if (wmax) w = wmax[r] + bias;
#pragma unroll
    for (int k = 0; k < NPT; ++k) e[k] = *(const float*)(row + col[k]);
  };
  auto emit = [&](int k, float w, const float* e) { return ((wild >> k) & 1u) ? w : e[k]; };

  float aT[NPT], aB[NPT], bstart;
  int f = q.f0;
  fill(eb, ew, et, row_of(f));
  if (f == 0) {
    bstart = eb;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      // -1 among the predecessors: bounded by the in-degree (frame 0 only)
      bool from_start = false;
      const int deg = (int)(meta[k] >> 16), a1 = (int)(meta[k] & 0xffffu);
      for (int a = 0; a < deg; ++a) from_start = from_start || ((a == 0 ? arc0[k] : arcs[a1 + a - 1]) & ARC_SLOT) == 0;
      aT[k] = from_start ? emit(k, ew, et) : NEG;
      aB[k] = NEG;
    }
    f = 1;
    fill(eb, ew, et, row_of(f));
  } else {
    bstart = alpha[0].y;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      const float2 v = j < N ? alpha[j + 1] : make_float2(NEG, NEG);
      aT[k] = v.x; aB[k] = v.y;
    }
  }
  int par = 0;
  auto publish = [&](int p) {
    float2* dst = pub + (size_t)p * slots_cap;
    if (tid == 0) dst[0] = make_float2(NEG, bstart);
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      if (j < N) dst[j + 1] = make_float2(aT[k], aB[k]);
    }
  };
  publish(0);
  __syncthreads();
  int rnext = row_of(f + 1);
  for (; f < q.f1; ++f) {
    float ebn, ewn = 0.f, etn[NPT];
    fill(ebn, ewn, etn, rnext);                    // frame f + 1's emissions: in flight across this frame's step and its barrier
    rnext = row_of(f + 2);
    const float2* src = pub + (size_t)par * slots_cap;
    uint8_t* bprow = bp + (size_t)f * q.bp_stride;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      const int deg = (int)(meta[k] >> 16), a1 = (int)(meta[k] & 0xffffu);
      if (deg > 0) {
        float best = aT[k];
        unsigned code = 0;
        unsigned arc = arc0[k];
        for (int a = 0; a < deg; ++a) {
          const float2 v = src[arc & ARC_SLOT];
          const float c = ((arc & ARC_T) && v.x > v.y) ? v.x : v.y;   // B_p, then T_p: the better of the pair, B_p on a tie
          if (c > best) { best = c; code = 1u + (unsigned)a; }
          if (a + 1 < deg) arc = arcs[a1 + a];
        }
        const bool bt = aT[k] > aB[k];             // B_j: stay, then T_j
        aB[k] = (bt ? aT[k] : aB[k]) + eb;
        aT[k] = best + emit(k, ew, et);
        bprow[j] = (uint8_t)(code | (bt ? 0x80u : 0u));
      }
    }
    bstart += eb;
    par ^= 1;
    publish(par);
    eb = ebn; ew = ewn;
#pragma unroll
    for (int k = 0; k < NPT; ++k) et[k] = etn[k];
    __syncthreads();
  }
  if (tid == 0) alpha[0] = make_float2(NEG, bstart);
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = tid + k * nth;
    if (j < N) alpha[j + 1] = make_float2(aT[k], aB[k]);
  }
}

// one lane per lattice: the end state over the finals, then T - 1 frames of dependent back-pointer loads.
// states[t] = 2 * slot + (1 on the token state), slot 0 = start, slot j + 1 = node j
__global__ void ctc_graph_backtrace_kernel(const GraphSeq* __restrict__ seqs, const int* __restrict__ arc_off_all,
                                           const unsigned* __restrict__ arcs_all, const int* __restrict__ finals_all,
                                           const float* __restrict__ alpha_all, const uint8_t* __restrict__ bp_all, int* __restrict__ states,
                                           float* __restrict__ score) {
  if (threadIdx.x != 0) return;
  const GraphSeq q = seqs[blockIdx.x];
  const float2* alpha = (const float2*)(alpha_all + q.alpha_off);
  const uint8_t* bp = bp_all + q.bp_off;
  const int* aoff = arc_off_all + q.node_off + q.index;
  const unsigned* arcs = arcs_all + q.arc_off;
  const int* fin = finals_all + q.fin_off;
  int* out = states + q.frame_off;
  float best = -INFINITY;
  int st = 2 * (fin[0] + 1);                       // no finite end: reported through the score
  for (int i = 0; i < q.n_final; ++i) {
    const float2 v = alpha[fin[i] + 1];
    if (v.y > best) { best = v.y; st = 2 * (fin[i] + 1); }
    if (v.x > best) { best = v.x; st = 2 * (fin[i] + 1) + 1; }
  }
  score[blockIdx.x] = best;
  for (int t = q.T - 1; t >= 1; --t) {
    out[t] = st;
    const int slot = st >> 1;
    if (slot == 0) continue;                       // B_start only stays
    const unsigned byte = bp[(size_t)t * q.bp_stride + slot - 1];
    if (st & 1) {
      const unsigned code = byte & 0x7fu;
      if (code) {
        const unsigned arc = arcs[aoff[slot - 1] + (int)code - 1];
        const int p = (int)(arc & ARC_SLOT);
        int from_t = 0;
        if (arc & ARC_T) from_t = bp[(size_t)t * q.bp_stride + p - 1] >> 7;   // T_p(t-1) > B_p(t-1): p's own blank bit
        st = 2 * p + from_t;
      }
    } else {
      st = 2 * slot + (int)(byte >> 7);
    }
  }
  out[0] = st;
}

constexpr int GRAPH_LDS_MAX = 2 * (CTC_GRAPH_MAX_NODES + 1) * (int)sizeof(float2);   // what an instantiation may be launched with

template <int NPT>
int launch_forward(hipStream_t s, int n_seq, int threads, size_t lds, const GraphSeq* seqs, const float* lp, int ld, int r0, const int* rows,
                   const int* node_tok, const int* arc_off, const unsigned* arcs, int blank, float* alpha, uint8_t* bp, const float* wmax,
                   float bias, int slots) {
  static bool attr_set = false;                    // once per instantiation, for the largest launch: not per slab
  if (!attr_set) {
    RVB_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_graph_forward_kernel<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, GRAPH_LDS_MAX));
    attr_set = true;
  }
  ctc_graph_forward_kernel<NPT><<<n_seq, threads, lds, s>>>(seqs, lp, ld, r0, rows, node_tok, arc_off, arcs, blank, alpha, bp, wmax, bias, slots);
  return OK;
}

}  // namespace

int ctc_graph_forward(hipStream_t s, const GraphSeq* seqs, int n_seq, int max_N, const float* lp, int ld, int r0, const int* rows,
                      const int* node_tok, const int* arc_off, const unsigned* arcs, int blank, float* alpha, uint8_t* bp,
                      const float* wmax, float bias) {
  if (n_seq <= 0) return OK;
  if (max_N < 1 || max_N > CTC_GRAPH_MAX_NODES) { set_error("ctc_graph_forward: nodes out of range"); return E_ARG; }
  const int npt = ctc_graph_npt_for(max_N);
  const int threads = ctc_threads(max_N, npt);
  const int slots = max_N + 1;
  const size_t lds = (size_t)2 * slots * sizeof(float2);
#define RVB_GRAPH_(NPT) RVB_TRY(launch_forward<NPT>(s, n_seq, threads, lds, seqs, lp, ld, r0, rows, node_tok, arc_off, arcs, blank, alpha, bp, wmax, bias, slots))
  if (npt == 1) RVB_GRAPH_(1);
  else if (npt == 2) RVB_GRAPH_(2);
  else if (npt == 4) RVB_GRAPH_(4);
  else RVB_GRAPH_(8);
#undef RVB_GRAPH_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int ctc_graph_backtrace(hipStream_t s, const GraphSeq* seqs, int n_seq, const int* arc_off, const unsigned* arcs, const int* finals,
                        const float* alpha, const uint8_t* bp, int* states, float* score) {
  if (n_seq <= 0) return OK;
  ctc_graph_backtrace_kernel<<<n_seq, 64, 0, s>>>(seqs, arc_off, arcs, finals, alpha, bp, states, score);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcGraphAligner::plan(const char* who, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds,
                          const uint8_t* is_final, int n_seq, const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id) {
  const std::string w(who);
  if (!node_tokens || !n_nodes || !pred_off || !preds || !is_final || n_seq <= 0 || (int)seq_rows.size() != n_seq) {
    set_error(w + ": null argument or no sequence");
    return E_ARG;
  }
  if (V < 2 || blank_id < 0 || blank_id >= V) { set_error(w + ": blank id outside [0, V)"); return E_ARG; }
  seq.assign(n_seq, GraphSeq{});
  h_tokens.clear(); h_arc_off.clear(); h_arcs.clear(); h_finals.clear(); h_rows.clear();
  max_N = 0; blank = blank_id; has_wild = false;
  size_t alpha_off = 0, bp_off = 0;
  int64_t node_off = 0, arc_off = 0, frame_off = 0;
  std::vector<int32_t> seen;                                    // per node of the lattice: the last node that listed it (duplicates)
  for (int i = 0; i < n_seq; ++i) {
    const int N = n_nodes[i];
    const int64_t T = (int64_t)seq_rows[i].size();
    const std::string at = w + ": sequence " + std::to_string(i) + ": ";
    if (N <= 0) { set_error(at + "empty graph (no node): nothing to align"); return E_ARG; }
    if (N > CTC_GRAPH_MAX_NODES) {
      set_error(at + std::to_string(N) + " nodes exceed the cap of " + std::to_string(CTC_GRAPH_MAX_NODES) + " nodes per graph");
      return E_UNSUPPORTED;
    }
    RVB_TRY(slab_frame_cap(at, T, CTC_ALIGN_MAX_FRAMES, "lattice"));
    const int32_t* y = node_tokens + node_off;
    const int32_t* po = pred_off + node_off + i;                 // N + 1 offsets, within this sequence's predecessors
    const int32_t* pr = preds + arc_off;
    const uint8_t* fin = is_final + node_off;
    if (po[0] != 0) { set_error(at + "pred_off must start at 0"); return E_ARG; }
    // the lists' sizes first: nothing below reads past a bad offset
    for (int j = 0; j < N; ++j) {
      const int64_t d = (int64_t)po[j + 1] - po[j];
      if (d <= 0) { set_error(at + "node " + std::to_string(j) + ": empty predecessor list"); return E_ARG; }
      if (d > CTC_GRAPH_MAX_IN_DEGREE) {
        set_error(at + "node " + std::to_string(j) + ": in-degree " + std::to_string(d) + " exceeds the cap of " +
                  std::to_string(CTC_GRAPH_MAX_IN_DEGREE) + " predecessors per node");
        return E_UNSUPPORTED;
      }
      if (po[j + 1] > CTC_GRAPH_MAX_ARCS) {
        set_error(at + "more than the cap of " + std::to_string(CTC_GRAPH_MAX_ARCS) + " arcs per graph (reached at node " + std::to_string(j) + ")");
        return E_UNSUPPORTED;
      }
    }
    seen.assign(N + 1, -1);
    bool any_final = false, any_start = false;
    const size_t fin0 = h_finals.size();
    for (int j = 0; j < N; ++j) {
      const std::string nd = at + "node " + std::to_string(j) + ": ";
      if (y[j] == RVB_CTC_WILDCARD) has_wild = true;
      else if (y[j] < 0 || y[j] >= V) { set_error(nd + "label " + std::to_string(y[j]) + " outside [0, " + std::to_string(V) + ")"); return E_ARG; }
      else if (y[j] == blank_id) { set_error(nd + "label is the blank id " + std::to_string(blank_id)); return E_ARG; }
      for (int a = po[j]; a < po[j + 1]; ++a) {
        const int p = pr[a];
        if (p < -1 || p >= j) {
          set_error(nd + "predecessor " + std::to_string(p) + " is not -1 (start) or an earlier node");
          return E_ARG;
        }
        if (seen[p + 1] == j) { set_error(nd + "duplicate predecessor " + std::to_string(p)); return E_ARG; }
        seen[p + 1] = j;
        if (p < 0) any_start = true;
        h_arcs.push_back((uint32_t)(p + 1) | ((p >= 0 && y[p] != y[j]) ? 0x8000u : 0u));
      }
      if (fin[j]) { any_final = true; h_finals.push_back(j); }
    }
    if (!any_final) { set_error(at + "no final node"); return E_ARG; }
    // defence only: node 0's non-empty list can hold nothing but -1, so a graph that passed the checks above has a start
    if (!any_start) { set_error(at + "no node with a start predecessor (-1)"); return E_ARG; }
    if (T < 1) { set_error(at + "infeasible: no frame"); return E_ARG; }
    GraphSeq& q = seq[i];
    q.N = N; q.T = (int)T; q.index = i;
    q.node_off = (int)node_off; q.arc_off = (int)arc_off; q.frame_off = (int)frame_off;
    q.fin_off = (int)fin0; q.n_final = (int)(h_finals.size() - fin0);
    const size_t n_pad = (size_t)(N + 63) / 64 * 64;             // layout independent of the instantiation chosen for the batch
    q.alpha_off = (long long)alpha_off; q.bp_off = (long long)bp_off; q.bp_stride = (long long)n_pad;
    alpha_off += 2 * (n_pad + 2);                               // {T, B} per slot, slot 0 = start; the offset stays 8-byte aligned
    bp_off += (size_t)T * n_pad;
    max_N = std::max(max_N, N);
    h_tokens.insert(h_tokens.end(), y, y + N);
    h_arc_off.insert(h_arc_off.end(), po, po + N + 1);
    node_off += N; arc_off += po[N];
    RVB_TRY(slab_take_rows(w, at, seq_rows[i], &h_rows, &frame_off, "frames or arcs"));
    if (arc_off > std::numeric_limits<int32_t>::max() / 2) { set_error(w + ": too many frames or arcs in one call"); return E_UNSUPPORTED; }
  }
  alpha_floats = alpha_off; bp_bytes = bp_off; total_frames = frame_off;
  return OK;
}

int CtcGraphAligner::begin(hipStream_t s) {
  RVB_TRY(d_tokens.ensure(h_tokens.size() * 4));
  RVB_TRY(d_arc_off.ensure(h_arc_off.size() * 4));
  RVB_TRY(d_arcs.ensure(h_arcs.size() * 4));
  RVB_TRY(d_finals.ensure(h_finals.size() * 4));
  RVB_TRY(d_rows.ensure(h_rows.size() * 4));
  RVB_TRY(d_seqs.ensure(seq.size() * sizeof(GraphSeq)));
  RVB_TRY(d_alpha.ensure(alpha_floats * 4));
  RVB_TRY(d_states.ensure((size_t)total_frames * 4));
  RVB_TRY(d_score.ensure(seq.size() * 4));
  if (int r = d_bp.ensure(bp_bytes)) {
    set_error("ctc align graph: " + std::to_string(bp_bytes) + " bytes of back-pointers (1 byte per frame and node) do not fit: " + last_error());
    return r;
  }
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), h_tokens.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_arc_off.p, h_arc_off.data(), h_arc_off.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_arcs.p, h_arcs.data(), h_arcs.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_finals.p, h_finals.data(), h_finals.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice, s));
  for (auto& q : seq) q.f0 = q.f1 = 0;
  return OK;
}

int CtcGraphAligner::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax, float bias) {
  if (has_wild && !wmax) { set_error("ctc align graph: a graph with wildcards needs the row maxima"); return E_ARG; }
  bool any;
  RVB_TRY(slab_window("ctc align graph", false, seq, h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, d_seqs.p, seq));
  return ctc_graph_forward(s, d_seqs.as<GraphSeq>(), (int)seq.size(), max_N, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(),
                           d_arc_off.as<int>(), d_arcs.as<unsigned>(), blank, d_alpha.as<float>(), d_bp.as<uint8_t>(),
                           has_wild ? wmax : nullptr, bias);
}

int CtcGraphAligner::finish(hipStream_t s, int32_t* states, float* score) {
  RVB_TRY(slab_covered("ctc align graph", false, seq));
  RVB_TRY(ctc_graph_backtrace(s, d_seqs.as<GraphSeq>(), (int)seq.size(), d_arc_off.as<int>(), d_arcs.as<unsigned>(), d_finals.as<int>(),
                               d_alpha.as<float>(), d_bp.as<uint8_t>(), d_states.as<int>(), d_score.as<float>()));
  RVB_HIP_CHECK(hipMemcpyAsync(states, d_states.p, (size_t)total_frames * 4, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipMemcpyAsync(score, d_score.p, seq.size() * 4, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  return slab_feasible("ctc align graph", seq, score, "through the graph ends in a final node");
}

void CtcGraphAligner::release() {
  for (DevBuf* b : {&d_tokens, &d_arc_off, &d_arcs, &d_finals, &d_rows, &d_seqs, &d_alpha, &d_bp, &d_states, &d_score}) b->release();
}

}  // namespace rvb
