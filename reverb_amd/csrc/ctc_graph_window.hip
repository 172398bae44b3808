// Windowed CTC Viterbi over a token GRAPH: alignment of a transcript with alternatives and optional words of any number of nodes over
// a lattice that arrives in several encoded batches.
//
// Graph, labels, predecessor lists, finals, the states B_start / T_j / B_j, the candidate order and the first-maximum rule are those
// of ctc_graph.hip.  What differs: at every frame only W consecutive nodes are alive, the window [lo, lo + W), and B_start only while
// lo == 0.  A predecessor below lo (the start, when lo > 0) is -inf, a node above every window so far still holds -inf, one below lo
// is never read again.  lo is a multiple of 64, never decreases and changes only BETWEEN launches (it is a field of the launch's
// descriptor), so inside a launch the kernel is ctc_graph_forward_kernel shifted by lo:
//
//   ownership    thread tid owns the nodes lo + tid + k * nthreads (NPT = 1 / 2 / 4 / 8 by ctc_graph_npt_for(W), up to 1024 threads)
//   LDS          slot j - lo + 1 holds node j's {T, B}, double-buffered: 2 x (W + 1) x 8 bytes (128 KiB + 16 B at the cap of 160 KiB).
//                Slot 0 is {-inf, B_start} when lo == 0 and {-inf, -inf} otherwise, and a predecessor p reads slot
//                max(p - lo + 1, 0): the band rule costs one max.
//   arcs         one 32-bit word RELATIVE to the node: the span j - p (j + 1 for the start, whose slot is then max(-lo, 0) = 0), the
//                allow-T bit, a marker on the node's LAST arc, which ends the loop over a list (the in-degree needs no register)
//                and, on a node's FIRST arc, whether any of its arcs is the start (all frame 0 asks); offsets are 32 bits.  The first arc of each owned node lives in a register,
//                the further ones are read from HBM through the L1 each frame.
//   alpha        {T, B} per slot of the WHOLE graph in HBM (slot 0 = start), -inf at begin(); a launch loads its window at its start
//                and stores it after its last frame.
//   back-ptrs    the one-byte code of ctc_graph.hip, window-relative: T x W bytes; lo_of[t] (int32 per frame, a plain vector store
//                of thread 0) tells the back-trace where frame t's row starts.
//   best         after its last frame the workgroup reduces its window to the FIRST maximum in the order B_start, T_lo, B_lo,
//                T_lo+1, ... (B_start reports node 0, no finite state reports -1): 8 bytes the host reads back to place the next
//                window and to choose the launch's length (ctc_graph_window_next).
//
// One workgroup, one __syncthreads() per frame, the next frame's emissions gathered before the barrier; every loop bounded by a frame
// count, a node count or an in-degree.  With W >= N the window never moves and labels, nodes and score are ctc_graph.hip's bit for
// bit, however the frames are cut; otherwise the result is the best path inside the windows.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace rvb {

namespace {

constexpr unsigned GW_SPAN = 0x1fffffffu, GW_ENTRY = 0x20000000u, GW_LAST = 0x40000000u, GW_T = 0x80000000u;
constexpr int GW_FAR = 1 << 30;                    // need[] of a node from which no final node is reached

struct GWinSeg {           // one launch: the lattice, its window and the frames to advance over
  int N, T, W;             // nodes, frames of the whole lattice, nodes of the window (a multiple of 64)
  int lo;                  // first node of the window (a multiple of 64; 0 in the launch that holds frame 0)
  int f0, f1;              // lattice frames this launch advances (f0 == 0: initialise; else continue from alpha in HBM)
  int fbase;               // the lattice frame of rows[0]: frame f reads row rows[f - fbase] - r0 of lp
};
struct GWinBest { int node; float value; };
struct GWinEnd { float score; int margin; int clamped; int pad_; };

template <int NPT>
__global__ __launch_bounds__(1024) void ctc_graph_window_kernel(const GWinSeg q, const float* __restrict__ lp, int ld, int r0,
                                                                const int* __restrict__ rows, const int* __restrict__ node_tok,
                                                                const int* __restrict__ aoff, const unsigned* __restrict__ arcs, int blank,
                                                                float* __restrict__ alpha_all, uint8_t* __restrict__ bp,
                                                                int* __restrict__ lo_of, GWinBest* __restrict__ best_out,
                                                                const float* __restrict__ wmax, float bias) {
  extern __shared__ __attribute__((aligned(16))) char gw_smem[];
  __shared__ float red_v[16];
  __shared__ unsigned red_k[16];
  float2* pub = (float2*)gw_smem;                  // [2][W + 1]: {T, B} of every slot, frames t - 1 and t
  if (q.f0 >= q.f1) return;                        // uniform over the workgroup
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = q.N, W = q.W, lo = q.lo, slots = W + 1;
  const float NEG = -INFINITY;
  float2* alpha = (float2*)alpha_all;              // [N + 1] slots of the whole graph

  unsigned col[NPT];                               // byte offset of the node's column in a row of lp (the blank's for a wildcard)
  unsigned arc0[NPT];                              // the node's first arc
  unsigned more[NPT];                              // where its further arcs start (0: no such node)
  unsigned wild = 0;                               // bit k: owned node k is a wildcard
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * nth, j = lo + i;       // window-relative and absolute
    col[k] = (unsigned)blank * 4u; arc0[k] = 0; more[k] = 0;
    if (i < W && j < N) {
      const int id = node_tok[j];
      if (id == RVB_CTC_WILDCARD) wild |= 1u << k; else col[k] = (unsigned)id * 4u;
      const int o = aoff[j];
      more[k] = (unsigned)o + 1u; arc0[k] = arcs[o];
    }
  }

  auto row_of = [&](int fr) { return rows[min(fr, q.f1 - 1) - q.fbase] - r0; };   // past the launch's last frame: clamped, in bounds
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
  if (f == 0) {                                    // the window of frame 0 starts at node 0
    bstart = eb;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      aT[k] = (arc0[k] & GW_ENTRY) ? emit(k, ew, et) : NEG;      // -1 among the predecessors: marked on the first arc
      aB[k] = NEG;
    }
    if (tid == 0) lo_of[0] = lo;
    f = 1;
    fill(eb, ew, et, row_of(f));
  } else {
    bstart = lo == 0 ? alpha[0].y : NEG;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const float2 v = more[k] ? alpha[lo + tid + k * nth + 1] : make_float2(NEG, NEG);
      aT[k] = v.x; aB[k] = v.y;
    }
  }
  int par = 0;
  auto publish = [&](int p) {
    float2* dst = pub + (size_t)p * slots;
    if (tid == 0) dst[0] = make_float2(NEG, bstart);
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      if (more[k]) dst[tid + k * nth + 1] = make_float2(aT[k], aB[k]);
  };
  publish(0);
  __syncthreads();
  int rnext = row_of(f + 1);
  for (; f < q.f1; ++f) {
    float ebn, ewn = 0.f, etn[NPT];
    fill(ebn, ewn, etn, rnext);                    // frame f + 1's emissions: in flight across this frame's step and its barrier
    rnext = row_of(f + 2);
    const float2* src = pub + (size_t)par * slots;
    uint8_t* bprow = bp + (size_t)f * W;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int i = tid + k * nth;
      if (more[k]) {
        float best = aT[k];
        unsigned code = 0;
        unsigned arc = arc0[k];
        for (int a = 0; a < CTC_GRAPH_MAX_IN_DEGREE; ++a) {
          const float2 v = src[max(i + 1 - (int)(arc & GW_SPAN), 0)];   // below the window, or the start with lo > 0: slot 0
          const float c = ((arc & GW_T) && v.x > v.y) ? v.x : v.y;     // B_p, then T_p: the better of the pair, B_p on a tie
          if (c > best) { best = c; code = 1u + (unsigned)a; }
          if (arc & GW_LAST) break;
          arc = arcs[more[k] + a];
        }
        const bool bt = aT[k] > aB[k];             // B_j: stay, then T_j
        aB[k] = (bt ? aT[k] : aB[k]) + eb;
        aT[k] = best + emit(k, ew, et);
        bprow[i] = (uint8_t)(code | (bt ? 0x80u : 0u));
      }
    }
    if (tid == 0) lo_of[f] = lo;
    bstart += eb;                                  // stays -inf where lo > 0
    par ^= 1;
    publish(par);
    eb = ebn; ew = ewn;
#pragma unroll
    for (int k = 0; k < NPT; ++k) et[k] = etn[k];
    __syncthreads();
  }
  // the window goes back to HBM, and its first maximum in the order B_start, T_lo, B_lo, T_lo+1, ... to the host
  float bv = NEG;
  unsigned bk = 0xffffffffu;                       // the place in that order; none: no finite state so far
  if (tid == 0 && lo == 0) {
    alpha[0] = make_float2(NEG, bstart);
    if (bstart > bv) { bv = bstart; bk = 0; }
  }
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * nth;
    if (more[k]) {
      alpha[lo + i + 1] = make_float2(aT[k], aB[k]);
      if (aT[k] > bv) { bv = aT[k]; bk = 1u + 2u * (unsigned)i; }         // i ascends with k: a later k only wins when greater
      if (aB[k] > bv) { bv = aB[k]; bk = 2u + 2u * (unsigned)i; }
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64);
    const unsigned k2 = __shfl_xor(bk, o, 64);
    if (v2 > bv || (v2 == bv && k2 < bk)) { bv = v2; bk = k2; }
  }
  if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_k[tid >> 6] = bk; }
  __syncthreads();
  if (tid == 0) {
    const int nw = nth >> 6;
    for (int w = 1; w < nw; ++w)
      if (red_v[w] > bv || (red_v[w] == bv && red_k[w] < bk)) { bv = red_v[w]; bk = red_k[w]; }
    best_out->node = bk == 0xffffffffu ? -1 : bk == 0 ? 0 : lo + (int)((bk - 1u) >> 1);
    best_out->value = bv;
  }
}

// one lane: the end state over the final nodes alive at the last frame, then T - 1 dependent back-pointer loads, each in the row of
// its own frame's window.  states[t] = 2 * slot + (1 on the token state), slot 0 = start, slot j + 1 = node j, as ctc_graph.hip's
__global__ void ctc_graph_window_backtrace_kernel(int N, int T, int W, const int* __restrict__ aoff, const unsigned* __restrict__ arcs,
                                                  const int* __restrict__ fin, int n_final, const float* __restrict__ alpha_all,
                                                  const uint8_t* __restrict__ bp, const int* __restrict__ lo_of, int* __restrict__ states,
                                                  GWinEnd* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float2* alpha = (const float2*)alpha_all;
  const int lo_end = lo_of[T - 1];
  float best = -INFINITY;
  int st = 2 * (fin[0] + 1);                       // no finite end: reported through the score
  for (int i = 0; i < n_final; ++i) {
    const int fj = fin[i];
    if (fj < lo_end || fj >= lo_end + W) continue; // below the window: stale; above it: -inf
    const float2 v = alpha[fj + 1];
    if (v.y > best) { best = v.y; st = 2 * (fj + 1); }
    if (v.x > best) { best = v.x; st = 2 * (fj + 1) + 1; }
  }
  int margin = W, clamped = 0;
  for (int t = T - 1; t >= 0; --t) {
    states[t] = st;
    const int slot = st >> 1;
    if (slot == 0) continue;                       // B_start only stays, and has no distance to an edge
    const int j = slot - 1, lo = lo_of[t];
    int idx = j - lo;
    if (idx < 0 || idx >= W) { clamped = 1; idx = min(max(idx, 0), W - 1); }       // cannot happen on a path with a finite score
    if (lo > 0) margin = min(margin, idx);                                        // the graph's own edges do not count
    if (lo + W < N) margin = min(margin, W - 1 - idx);
    if (t == 0) break;
    const unsigned byte = bp[(size_t)t * W + idx];
    if (st & 1) {
      const unsigned code = byte & 0x7fu;
      if (code) {
        const unsigned arc = arcs[aoff[j] + (int)code - 1];
        const int p = j - (int)(arc & GW_SPAN);    // -1: the start
        int from_t = 0;
        if (p >= 0 && (arc & GW_T)) {
          int pi = p - lo;
          if (pi < 0 || pi >= W) { clamped = 1; pi = min(max(pi, 0), W - 1); }
          from_t = bp[(size_t)t * W + pi] >> 7;    // T_p(t-1) > B_p(t-1): p's own blank bit, in the same frame's row
        }
        st = 2 * (p + 1) + from_t;
      }
    } else {
      st = 2 * slot + (int)(byte >> 7);
    }
  }
  out->score = best;
  out->margin = margin;
  out->clamped = clamped;
}

constexpr int GWIN_LDS_MAX = 2 * (CTC_GRAPH_WINDOW_MAX_NODES + 1) * (int)sizeof(float2);   // what an instantiation may be launched with
static_assert(GWIN_LDS_MAX + 16 * 8 <= 160 * 1024, "the window's two rows of {T, B} and the reduction fit one workgroup's LDS");

template <int NPT>
int launch_window(hipStream_t s, int threads, size_t lds, const GWinSeg& q, const float* lp, int ld, int r0, const int* rows,
                  const int* node_tok, const int* aoff, const unsigned* arcs, int blank, float* alpha, uint8_t* bp, int* lo_of,
                  GWinBest* best, const float* wmax, float bias) {
  static bool attr_set = false;                    // once per instantiation, for the largest launch: not per launch
  if (!attr_set) {
    RVB_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_graph_window_kernel<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, GWIN_LDS_MAX));
    attr_set = true;
  }
  ctc_graph_window_kernel<NPT><<<1, threads, lds, s>>>(q, lp, ld, r0, rows, node_tok, aoff, arcs, blank, alpha, bp, lo_of, best, wmax, bias);
  return OK;
}

int graph_window_forward(hipStream_t s, const GWinSeg& q, const float* lp, int ld, int r0, const int* rows, const int* node_tok,
                         const int* aoff, const unsigned* arcs, int blank, float* alpha, uint8_t* bp, int* lo_of, GWinBest* best,
                         const float* wmax, float bias) {
  if (q.W < 64 || q.W > CTC_GRAPH_WINDOW_MAX_NODES || q.W % 64 != 0 || q.lo < 0 || q.lo % 64 != 0) {
    set_error("ctc_graph_window: window out of range");
    return E_ARG;
  }
  const int npt = ctc_graph_npt_for(q.W), threads = ctc_threads(q.W, npt);
  const size_t lds = (size_t)2 * (q.W + 1) * sizeof(float2);
#define RVB_GWIN_(NPT) RVB_TRY(launch_window<NPT>(s, threads, lds, q, lp, ld, r0, rows, node_tok, aoff, arcs, blank, alpha, bp, lo_of, best, wmax, bias))
  if (npt == 1) RVB_GWIN_(1);
  else if (npt == 2) RVB_GWIN_(2);
  else if (npt == 4) RVB_GWIN_(4);
  else RVB_GWIN_(8);
#undef RVB_GWIN_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int pad64(int v) { return (v + 63) / 64 * 64; }
int floor64(int v) { return v >= 0 ? v / 64 * 64 : -((-v + 63) / 64 * 64); }

}  // namespace

// ------------------------------------------------------------------------------------ the window policy (host only, pure)
CtcGraphWindowStep ctc_graph_window_next(const CtcGraphWindowTables& g, int T, int W, int f0, int fend, int lo_prev, int best_prev) {
  const int N = g.N, top = std::max(0, pad64(N) - W);
  int lo, c;
  if (f0 <= 0) {                                                          // 1. the first launch: frame 0 lives in the start's successors
    lo = 0; c = g.startmax;
  } else {
    lo = best_prev >= 0 ? floor64(best_prev - W / 2) : lo_prev;           //    else centre on the best node (none finite: stay),
    lo = std::min(std::max(std::max(lo, lo_prev), 0), top);               //    never back, never past the graph's end
    c = std::max(best_prev, lo);
  }
  int f1 = f0;                                                            // 2. the launch lasts for as long as the climber (the highest
  while (f1 < fend) {                                                     //    node the best partial path can have reached) stays inside
    const int nc = f1 > 0 ? g.M[c] : c;
    if (f1 > f0 && lo + W < N && nc > lo + W - 1) break;
    c = nc;
    ++f1;
  }
  const int r = T - f1;                                                   // 3. at frame f1 - 1 the window still reaches a node from which
  const int e = g.E[std::min<size_t>((size_t)std::max(r, 0), g.E.size() - 1)];   // a final one is r frames away
  if (lo + W - 1 < e) lo = std::min(pad64(e - W + 1), top);
  return {lo, f1};
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcGraphWindowAligner::plan(const char* who, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                const uint8_t* is_final, int64_t total_frames, int window_nodes, int V, int blank_id, float wildcard_bias) {
  const std::string w(who), at = w + ": ";
  open = false;
  if (!node_tokens || !pred_off || !preds || !is_final) { set_error(w + ": null argument"); return E_ARG; }
  if (V < 2 || blank_id < 0 || blank_id >= V) { set_error(w + ": blank id outside [0, V)"); return E_ARG; }
  if (!(std::isfinite(wildcard_bias) && wildcard_bias <= 0.f)) { set_error(w + ": wildcard_bias must be finite and <= 0"); return E_ARG; }
  if (window_nodes != 0 && (window_nodes < 256 || window_nodes > CTC_GRAPH_WINDOW_MAX_NODES || window_nodes % 256 != 0)) {
    set_error(at + "window_nodes " + std::to_string(window_nodes) + " must be 0 (the default, " + std::to_string(CTC_GRAPH_WINDOW_DEFAULT_NODES) +
              ") or a multiple of 256 in [256, " + std::to_string(CTC_GRAPH_WINDOW_MAX_NODES) + "]");
    return E_ARG;
  }
  const int N_ = n_nodes;
  if (N_ <= 0) { set_error(at + "empty graph (no node): nothing to align"); return E_ARG; }
  if (total_frames < 1) { set_error(at + "infeasible: no frame"); return E_ARG; }
  RVB_TRY(slab_frame_cap(at, total_frames, CTC_ALIGN_MAX_FRAMES, "lattice"));
  const int32_t* y = node_tokens;
  const int32_t* po = pred_off;
  if (po[0] != 0) { set_error(at + "pred_off must start at 0"); return E_ARG; }
  // the lists' sizes first: nothing below reads past a bad offset
  for (int j = 0; j < N_; ++j) {
    const int64_t d = (int64_t)po[j + 1] - po[j];
    if (d <= 0) { set_error(at + "node " + std::to_string(j) + ": empty predecessor list"); return E_ARG; }
    if (d > CTC_GRAPH_MAX_IN_DEGREE) {
      set_error(at + "node " + std::to_string(j) + ": in-degree " + std::to_string(d) + " exceeds the cap of " +
                std::to_string(CTC_GRAPH_MAX_IN_DEGREE) + " predecessors per node");
      return E_UNSUPPORTED;
    }
  }
  h_tokens.assign(y, y + N_);
  h_arc_off.assign(po, po + N_ + 1);
  h_arcs.clear(); h_finals.clear();
  h_arcs.reserve((size_t)po[N_]);
  has_wild = false;
  CtcGraphWindowTables& g = tab;
  g.N = N_; g.startmax = -1;
  g.M.resize((size_t)N_);
  for (int j = 0; j < N_; ++j) g.M[j] = j;
  std::vector<int32_t> seen((size_t)N_ + 1, -1);                   // per node: the last node that listed it (duplicates)
  int span = 0, span_node = 0;
  for (int j = 0; j < N_; ++j) {
    const std::string nd = at + "node " + std::to_string(j) + ": ";
    if (y[j] == RVB_CTC_WILDCARD) has_wild = true;
    else if (y[j] < 0 || y[j] >= V) { set_error(nd + "label " + std::to_string(y[j]) + " outside [0, " + std::to_string(V) + ")"); return E_ARG; }
    else if (y[j] == blank_id) { set_error(nd + "label is the blank id " + std::to_string(blank_id)); return E_ARG; }
    for (int a = po[j]; a < po[j + 1]; ++a) {
      const int p = preds[a];
      if (p < -1 || p >= j) {
        set_error(nd + "predecessor " + std::to_string(p) + " is not -1 (start) or an earlier node");
        return E_ARG;
      }
      if (seen[p + 1] == j) { set_error(nd + "duplicate predecessor " + std::to_string(p)); return E_ARG; }
      seen[p + 1] = j;
      if (p < 0) g.startmax = j; else g.M[p] = std::max(g.M[p], j);
      if (j - p > span) { span = j - p; span_node = j; }
      h_arcs.push_back((uint32_t)(j - p) | (a + 1 == po[j + 1] ? GW_LAST : 0u) | ((p >= 0 && y[p] != y[j]) ? GW_T : 0u));
      if (p < 0) h_arcs[(size_t)po[j]] |= GW_ENTRY;
    }
    if (is_final[j]) h_finals.push_back(j);
  }
  if (h_finals.empty()) { set_error(at + "no final node"); return E_ARG; }
  // defence only: node 0's non-empty list can hold nothing but -1, so a graph that passed the checks above has a start
  if (g.startmax < 0) { set_error(at + "no node with a start predecessor (-1)"); return E_ARG; }
  for (int j = 1; j < N_; ++j) g.M[j] = std::max(g.M[j], g.M[j - 1]);
  // need[j]: the fewest further frames from T_j to a final node; an arc between equal labels costs two, the blank between them.
  // A node relaxes its predecessors once it is final itself: descending order visits every successor before the node.
  std::vector<int32_t> need((size_t)N_, GW_FAR);
  for (int f : h_finals) need[f] = 0;
  int shortest = GW_FAR, need_top = 0;
  for (int j = N_ - 1; j >= 0; --j) {
    if (need[j] >= GW_FAR) continue;
    need_top = std::max(need_top, need[j]);
    for (int a = po[j]; a < po[j + 1]; ++a) {
      const int p = preds[a];
      if (p < 0) shortest = std::min(shortest, need[j] + 1);
      else if (!is_final[p]) need[p] = std::min(need[p], need[j] + (y[p] != y[j] ? 1 : 2));
    }
  }
  if (shortest >= GW_FAR) { set_error(at + "no final node is reached from the start"); return E_ARG; }
  if (total_frames < shortest) {
    set_error(at + "infeasible: the graph's shortest reading needs at least " + std::to_string(shortest) + " frames, the lattice has " +
              std::to_string(total_frames));
    return E_ARG;
  }
  g.E.assign((size_t)need_top + 1, N_);
  for (int j = N_ - 1; j >= 0; --j)
    if (need[j] < GW_FAR) g.E[need[j]] = j;
  for (size_t r = 1; r < g.E.size(); ++r) g.E[r] = std::min(g.E[r], g.E[r - 1]);
  N = N_; T = (int)total_frames;
  W = std::min(window_nodes ? window_nodes : (int)CTC_GRAPH_WINDOW_DEFAULT_NODES, pad64(N));
  if (W < N && span > W / 2 - 64) {
    set_error(at + "node " + std::to_string(span_node) + ": an arc of span " + std::to_string(span) + " nodes exceeds what a window of " +
              std::to_string(W) + " nodes follows (" + std::to_string(W / 2 - 64) + "): ask for a wider window");
    return E_UNSUPPORTED;
  }
  blank = blank_id; bias = wildcard_bias;
  bp_bytes = (size_t)T * (size_t)W;
  h_rows.clear();
  fed = fbase = 0; lo = 0; best = -1; launches = 0;
  lo_force = nullptr; n_force = 0;
  return OK;
}

int CtcGraphWindowAligner::begin(hipStream_t s) {
  RVB_TRY(d_tokens.ensure((size_t)N * 4));
  RVB_TRY(d_arc_off.ensure(((size_t)N + 1) * 4));
  RVB_TRY(d_arcs.ensure(h_arcs.size() * 4));
  RVB_TRY(d_finals.ensure(h_finals.size() * 4));
  RVB_TRY(d_alpha.ensure(((size_t)N + 1) * 8));
  RVB_TRY(d_lo.ensure((size_t)T * 4));
  RVB_TRY(d_states.ensure((size_t)T * 4));
  RVB_TRY(d_best.ensure(sizeof(GWinBest)));
  RVB_TRY(d_end.ensure(sizeof(GWinEnd)));
  if (int r = d_bp.ensure(bp_bytes)) {
    set_error("ctc align graph long: " + std::to_string(bp_bytes) + " bytes of back-pointers (1 byte per frame and window node) do not fit: " +
              last_error());
    return r;
  }
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_arc_off.p, h_arc_off.data(), ((size_t)N + 1) * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_arcs.p, h_arcs.data(), h_arcs.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_finals.p, h_finals.data(), h_finals.size() * 4, hipMemcpyHostToDevice, s));
  const float ninf = -INFINITY;
  int bits;
  memcpy(&bits, &ninf, 4);
  RVB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_alpha.p, bits, ((size_t)N + 1) * 2, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));          // the host vectors may be replaced by the next plan()
  open = true;
  return OK;
}

int CtcGraphWindowAligner::batch(hipStream_t s, const std::vector<int32_t>& rows) {
  if (!open) { set_error("ctc align graph long: feed before begin"); return E_STATE; }
  if (fed != fbase + (int64_t)h_rows.size()) { set_error("ctc align graph long: the slabs did not cover every frame of the batch before"); return E_STATE; }
  if (fed + (int64_t)rows.size() > T) {
    set_error("ctc align graph long: feed after the lattice's frames are used up: " + std::to_string(fed) + " of " + std::to_string(T) +
              " frames fed, the batch holds " + std::to_string(rows.size()) + " more");
    return E_STATE;
  }
  for (size_t f = 1; f < rows.size(); ++f)
    if (rows[f] <= rows[f - 1]) { set_error("ctc align graph long: frame rows must increase"); return E_ARG; }
  h_rows = rows;
  fbase = fed;
  RVB_TRY(d_rows.ensure(std::max<size_t>(rows.size(), 1) * 4));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  RVB_HIP_CHECK(hipMemcpy(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice));
  return OK;
}

bool CtcGraphWindowAligner::touches(int r0, int nrows) const {
  const auto a = std::lower_bound(h_rows.begin(), h_rows.end(), r0), b = std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows);
  return a != b;
}

int CtcGraphWindowAligner::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows, const float* wmax) {
  if (!open) { set_error("ctc align graph long: feed before begin"); return E_STATE; }
  if (has_wild && !wmax) { set_error("ctc align graph long: a graph with wildcards needs the row maxima"); return E_ARG; }
  const int b0 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0) - h_rows.begin());
  const int b1 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows) - h_rows.begin());
  if (b0 == b1) return OK;
  if (fbase + b0 != fed) { set_error("ctc align graph long: slabs must arrive in row order"); return E_STATE; }
  for (int g0 = fbase + b0, end = fbase + b1; g0 < end;) {
    int g1;
    if (lo_force) {                                // lab hook: a slab is one launch, in the window given for it
      if (launches >= n_force) { set_error("ctc align graph long: more launches than forced windows"); return E_STATE; }
      lo = lo_force[launches]; g1 = end;
    } else {
      const CtcGraphWindowStep st = ctc_graph_window_next(tab, T, W, g0, end, lo, best);
      lo = st.lo; g1 = st.f1;
    }
    if (g1 <= g0 || g1 > end || lo < 0 || lo % 64 != 0 || lo > std::max(0, pad64(N) - W) || (g0 == 0 && lo != 0)) {
      set_error("ctc align graph long: the window policy left its bounds");
      return E_HIP;
    }
    GWinSeg q{N, T, W, lo, g0, g1, fbase};
    RVB_TRY(graph_window_forward(s, q, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), d_arc_off.as<int>(), d_arcs.as<unsigned>(), blank,
                                 d_alpha.as<float>(), d_bp.as<uint8_t>(), d_lo.as<int>(), d_best.as<GWinBest>(), has_wild ? wmax : nullptr,
                                 bias));
    GWinBest hb;
    RVB_HIP_CHECK(hipMemcpyAsync(&hb, d_best.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    RVB_HIP_CHECK(hipStreamSynchronize(s));        // the one synchronisation of a launch: the next window depends on it
    best = hb.node;
    fed = g1;
    g0 = g1;
    ++launches;
  }
  return OK;
}

int CtcGraphWindowAligner::finish(hipStream_t s, int32_t* states, float* score, int32_t* min_margin, int32_t* lo_out) {
  if (!open) { set_error("ctc align graph long: finish before begin"); return E_STATE; }
  if (fed != T) {
    set_error("ctc align graph long: finish before all " + std::to_string(T) + " frames were fed (" + std::to_string(fed) + " so far)");
    return E_STATE;
  }
  ctc_graph_window_backtrace_kernel<<<1, 64, 0, s>>>(N, T, W, d_arc_off.as<int>(), d_arcs.as<unsigned>(), d_finals.as<int>(),
                                                     (int)h_finals.size(), d_alpha.as<float>(), d_bp.as<uint8_t>(), d_lo.as<int>(),
                                                     d_states.as<int>(), d_end.as<GWinEnd>());
  RVB_HIP_CHECK(hipGetLastError());
  GWinEnd he;
  std::vector<int32_t> st((size_t)T), lo_host(lo_out ? (size_t)T : 0);
  RVB_HIP_CHECK(hipMemcpyAsync(st.data(), d_states.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  if (lo_out) RVB_HIP_CHECK(hipMemcpyAsync(lo_host.data(), d_lo.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipMemcpyAsync(&he, d_end.p, sizeof(he), hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  if (!(he.score > -INFINITY)) {
    set_error("ctc align graph long: infeasible: no path inside the window of " + std::to_string(W) + " nodes ends in a final node after " +
              std::to_string(T) + " frames with a finite score");
    return E_ARG;
  }
  if (he.clamped) { set_error("ctc align graph long: the back-trace left its window on a path with a finite score"); return E_HIP; }
  memcpy(states, st.data(), (size_t)T * 4);        // nothing is written before the last check: a refusal leaves the outputs untouched
  if (lo_out) memcpy(lo_out, lo_host.data(), (size_t)T * 4);
  if (score) *score = he.score;
  if (min_margin) *min_margin = he.margin;
  return OK;
}

void CtcGraphWindowAligner::release() {
  for (DevBuf* b : {&d_tokens, &d_arc_off, &d_arcs, &d_finals, &d_rows, &d_alpha, &d_bp, &d_lo, &d_best, &d_states, &d_end}) b->release();
  open = false;
}

}  // namespace rvb
