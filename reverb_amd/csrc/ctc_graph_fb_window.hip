// Windowed CTC full sum over a token GRAPH: the full-sum score (and per-node posteriors) of a transcript with alternatives of any number
// of nodes over a lattice that arrives in several encoded batches.  The eighth lattice: the recurrences, states, normalisation and
// per-node reductions of ctc_graph_score.hip, inside the window mechanics of ctc_graph_window.hip, by the windowed forward-backward
// protocol of ctc_fb_window.hip.
//
// Recurrences (ctc_graph_score.hip): states B_start, T_j, B_j; a^ = alpha - C[t] and b^ = beta - (loglik - C[t]) carried in fp64
// (registers, LDS, HBM), dlse2 / dlse3 with fp32 transcendentals, c[t] an fp32 value summed in fp64 by thread 0; gamma, visit,
// occupancy, frame-weighted sum and peak as there.
//
// Band semantics (restated in fp64 by tests/graph_score_window_ref.py).  lo_of[t] is the window of the launch that computes frame t: a
// multiple of 64 that never decreases.
//   * node j is alive at t iff lo_of[t] <= j < min(lo_of[t] + W, N); B_start is alive iff lo_of[t] == 0;
//   * a transition into T_j at t from predecessor p counts iff j is alive at t and p >= lo_of[t] (p = -1: iff lo_of[t] == 0);
//   * stay transitions of an alive node always count; a node that was not alive before holds -inf;
//   * loglik is the lse over the final nodes alive at the last frame, the posteriors are those of that sum.
//
// Window mechanics (ctc_graph_window.hip): lo is a field of the launch's descriptor; thread tid owns the nodes lo + tid + k * nthreads
// (NPT = 1 / 2 / 4 by ctc_graph_npt_for(W)); arcs are 32-bit words relative to the node (the span, allow-T, last-of-list, and on the
// first arc whether the node has a start arc), the first in a register, the further ones read through the L1; alpha and beta of the
// WHOLE graph live in HBM as double2 [N + 1] (slot 0 = start), -inf at begin(): a launch loads its window at its start and stores it
// at its end.
//   LDS        forward: slot j - lo + 1 holds node j's {T, B} as double2, double-buffered: 2 x (W + 1) x 16 bytes (131 104 B at the cap
//              of 4096 nodes).  Slot 0 is {-inf, B_start} when lo == 0 and {-inf, -inf} otherwise; predecessor p reads slot
//              max(p - lo + 1, 0).  Backward: T alone, 2 x W x 8 bytes.
//   live set   c[t] is the maximum of row t - 1 over the alive states that can still reach a final end in the frames left: per node
//              two 32-bit words (fewest frames from T_j / from B_j to a final end), one more word for B_start.
//   best       after its last frame the forward launch reduces its window, over those states, to the FIRST maximum of the normalised row
//              in the order B_start, T_lo, B_lo, T_lo+1, ... (B_start reports node 0, no finite state reports -1): 8 bytes the host
//              reads back for ctc_graph_window_next.
//   rows       with posteriors the forward launch stores a^(T_j) in fp32 WINDOW-RELATIVE (T x W x 4 bytes), c[t] and lo_of[t].
//   backward   replays the recorded launches in reverse, each with its own lo, over the transposed (successor) arcs.  At the launch's
//              first step (frame f1 - 1) after a move every node below lo_next gets -inf in both states (the mirror image of the forward
//              cut), and for that one step a successor in [lo + W, lo_next + W) reads its b^(T) from HBM; after it such a successor is
//              -inf.  The per-node reductions live in registers of the owning thread and in HBM between launches: no atomics.
//
// One workgroup, one __syncthreads() per frame, the next frame's emissions gathered before the barrier; every loop bounded by a frame
// count, a node count or a degree.  With W >= N rounded up to 64 the window never moves and loglik and the five per-node outputs are
// ctc_graph_score.hip's bit for bit, however the frames are cut: the accumulations are written in that kernel's form.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace rvb {

namespace {

// the arc words of ctc_graph_window.hip (engine.h: CtcGraphWindowAligner::h_arcs); the successor words use SPAN, LAST and T alike
constexpr unsigned GS_SPAN = 0x1fffffffu, GS_ENTRY = 0x20000000u, GS_LAST = 0x40000000u, GS_T = 0x80000000u;
constexpr unsigned GS_FAR = 1u << 30;              // frames to the end of a state that reaches no final node

struct GswSeg {            // one launch: the lattice, its window and the frames to advance over
  int N, T, W;             // nodes, frames of the whole lattice, nodes of the window (a multiple of 64)
  int lo;                  // first node of the window (a multiple of 64; 0 in the launch that holds frame 0)
  int lo_next;             // backward only: the window of the launch that owns frame f1 (lo when f1 == T)
  int f0, f1;              // lattice frames of this launch (forward: f0 == 0 initialises; backward: f1 == T starts the sweep)
  int fbase;               // the lattice frame of rows[0]: frame f reads row rows[f - fbase] - r0 of lp
};
struct GswBest { int node; float value; };

// ctc_graph_score.hip's, verbatim
__device__ __forceinline__ double dlse3(double x0, double x1, double x2) {
  const double m = fmax(fmax(x0, x1), x2);
  const double mm = m > -INFINITY ? m : 0.0;
  return mm + (double)logf(expf((float)(x0 - mm)) + expf((float)(x1 - mm)) + expf((float)(x2 - mm)));
}
__device__ __forceinline__ double dlse2(double x0, double x1) {
  const double m = fmax(x0, x1);
  const double mm = m > -INFINITY ? m : 0.0;
  return mm + (double)logf(expf((float)(x0 - mm)) + expf((float)(x1 - mm)));
}

template <int NPT>
__global__ __launch_bounds__(1024) void ctc_graph_fb_window_forward_kernel(const GswSeg q, const float* __restrict__ lp, int ld, int r0,
                                                                           const int* __restrict__ rows, const int* __restrict__ node_tok,
                                                                           const int* __restrict__ aoff, const unsigned* __restrict__ arcs,
                                                                           const unsigned* __restrict__ rem, int blank,
                                                                           double* __restrict__ alpha_all, double* __restrict__ csum,
                                                                           float* __restrict__ coff, float* __restrict__ arows,
                                                                           int* __restrict__ lo_of, GswBest* __restrict__ best_out) {
  extern __shared__ __attribute__((aligned(16))) char gsw_smem[];
  double2* pub = (double2*)gsw_smem;               // [2][W + 1]: {T, B} of every slot, frames t - 1 and t
  __shared__ float wmx[2][16];                     // per wave: maximum of the row over the live states
  __shared__ double red_v[16];
  __shared__ unsigned red_k[16];
  if (q.f0 >= q.f1) return;                        // uniform over the workgroup
  const int tid = threadIdx.x, nth = blockDim.x, nw = nth >> 6;
  const int N = q.N, W = q.W, lo = q.lo, slots = W + 1;
  const float NEG = -INFINITY;
  double2* alpha = (double2*)alpha_all;            // [N + 1] slots of the whole graph

  unsigned col[NPT];                               // byte offset of the node's column in a row of lp
  unsigned arc0[NPT];                              // the node's first arc
  unsigned more[NPT];                              // where its further arcs start (0: no such node)
  unsigned rmT[NPT], rmB[NPT];                     // frames to the end from T_j / from B_j
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * nth, j = lo + i;       // window-relative and absolute
    col[k] = (unsigned)blank * 4u; arc0[k] = 0; more[k] = 0; rmT[k] = GS_FAR; rmB[k] = GS_FAR;
    if (i < W && j < N) {
      col[k] = (unsigned)node_tok[j] * 4u;
      const int o = aoff[j];
      more[k] = (unsigned)o + 1u; arc0[k] = arcs[o];
      rmT[k] = rem[2 * j]; rmB[k] = rem[2 * j + 1];
    }
  }
  const unsigned rem_start = lo == 0 ? rem[2 * N] : GS_FAR;      // B_start is alive only while lo == 0

  auto row_of = [&](int fr) { return rows[min(fr, q.f1 - 1) - q.fbase] - r0; };   // past the launch's last frame: clamped, in bounds
  float eb, et[NPT];
  auto fill = [&](int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
#pragma unroll
    for (int k = 0; k < NPT; ++k) et[k] = *(const float*)(row + col[k]);
  };

  double aT[NPT], aB[NPT], bstart;
  int par = 0;
  auto publish = [&](int fr) {                     // the row of frame fr, just computed, and its maximum over the live states
    double2* dst = pub + (size_t)par * slots;
    const unsigned left = (unsigned)(q.T - 1 - fr);
    float m = NEG;
    if (tid == 0) { dst[0] = make_double2(NEG, bstart); if (rem_start <= left) m = (float)bstart; }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      if (more[k]) {
        dst[tid + k * nth + 1] = make_double2(aT[k], aB[k]);
        m = fmaxf(m, rmT[k] <= left ? (float)aT[k] : NEG);
        m = fmaxf(m, rmB[k] <= left ? (float)aB[k] : NEG);
      }
    }
    m = wave_max(m);
    if ((tid & 63) == 0) wmx[par][tid >> 6] = m;
    __syncthreads();
  };
  auto store_row = [&](int fr) {
    if (tid == 0) lo_of[fr] = lo;
    if (!arows) return;
    float* dst = arows + (size_t)fr * W;
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      if (more[k]) dst[tid + k * nth] = (float)aT[k];
  };

  int f = q.f0;
  double C = 0.0;
  fill(row_of(f));
  if (f == 0) {                                    // the window of frame 0 starts at node 0
    bstart = eb;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      aT[k] = (arc0[k] & GS_ENTRY) ? et[k] : NEG;  // -1 among the predecessors: marked on the first arc
      aB[k] = NEG;
    }
    if (tid == 0 && coff) coff[0] = 0.f;
    store_row(0);
    f = 1;
    fill(row_of(1));
  } else {
    bstart = lo == 0 ? alpha[0].y : NEG;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const double2 v = more[k] ? alpha[lo + tid + k * nth + 1] : make_double2(NEG, NEG);
      aT[k] = v.x; aB[k] = v.y;
    }
    if (tid == 0) C = csum[0];
  }
  publish(f - 1);

  for (; f < q.f1; ++f) {
    const char* rown = (const char*)(lp + (size_t)row_of(f + 1) * ld);   // frame f + 1's emissions: loaded as this frame's are used up
    const double2* src = pub + (size_t)par * slots;
    float m = wmx[par][0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, wmx[par][w]);
    const float c = m > NEG ? m : 0.f;             // the offset of this frame: the maximum of the row before it
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      if (more[k]) {
        const int i1 = tid + k * nth + 1;
        const double2 v0 = src[max(i1 - (int)(arc0[k] & GS_SPAN), 0)];       // below the window, or the start with lo > 0: slot 0
        const double x1 = v0.y, x2 = (arc0[k] & GS_T) ? v0.x : (double)NEG;
        double t;
        if (arc0[k] & GS_LAST) {
          t = dlse3(aT[k], x1, x2);
        } else {
          const unsigned* al = arcs + more[k];
          double mx = fmax(aT[k], fmax(x1, x2));
          for (int a = 0; a < CTC_GRAPH_MAX_IN_DEGREE - 1; ++a) {
            const unsigned arc = al[a];
            const double2 v = src[max(i1 - (int)(arc & GS_SPAN), 0)];
            mx = fmax(mx, fmax(v.y, (arc & GS_T) ? v.x : (double)NEG));
            if (arc & GS_LAST) break;
          }
          const double mm = mx > NEG ? mx : 0.0;
          float s = expf((float)(aT[k] - mm)) + expf((float)(x1 - mm)) + expf((float)(x2 - mm));
          for (int a = 0; a < CTC_GRAPH_MAX_IN_DEGREE - 1; ++a) {
            const unsigned arc = al[a];
            const double2 v = src[max(i1 - (int)(arc & GS_SPAN), 0)];
            s += expf((float)(v.y - mm));
            if (arc & GS_T) s += expf((float)(v.x - mm));
            if (arc & GS_LAST) break;
          }
          t = mm + (double)logf(s);
        }
        aB[k] = (dlse2(aB[k], aT[k]) + (double)eb) - (double)c;
        aT[k] = (t + (double)et[k]) - (double)c;
        et[k] = *(const float*)(rown + col[k]);
      }
    }
    bstart = (bstart + (double)eb) - (double)c;    // stays -inf where lo > 0
    eb = *(const float*)(rown + (unsigned)blank * 4u);
    if (tid == 0) { C += (double)c; if (coff) coff[f] = c; }
    store_row(f);
    par ^= 1;
    publish(f);
  }
  if (tid == 0) csum[0] = C;

  // the window goes back to HBM, and the first maximum of its last row over the live states, in the order B_start, T_lo, B_lo, ...
  const unsigned left = (unsigned)(q.T - q.f1);
  double bv = (double)NEG;
  unsigned bk = 0xffffffffu;                       // the place in that order; none: no finite live state
  if (tid == 0 && lo == 0) {
    alpha[0] = make_double2(NEG, bstart);
    if (rem_start <= left && bstart > bv) { bv = bstart; bk = 0; }
  }
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * nth;
    if (more[k]) {
      alpha[lo + i + 1] = make_double2(aT[k], aB[k]);
      if (rmT[k] <= left && aT[k] > bv) { bv = aT[k]; bk = 1u + 2u * (unsigned)i; }   // i ascends with k: a later k only wins when greater
      if (rmB[k] <= left && aB[k] > bv) { bv = aB[k]; bk = 2u + 2u * (unsigned)i; }
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double v2 = __shfl_xor(bv, o, 64);
    const unsigned k2 = __shfl_xor(bk, o, 64);
    if (v2 > bv || (v2 == bv && k2 < bk)) { bv = v2; bk = k2; }
  }
  if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_k[tid >> 6] = bk; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < nw; ++w)
      if (red_v[w] > bv || (red_v[w] == bv && red_k[w] < bk)) { bv = red_v[w]; bk = red_k[w]; }
    best_out->node = bk == 0xffffffffu ? -1 : bk == 0 ? 0 : lo + (int)((bk - 1u) >> 1);
    best_out->value = (float)bv;
  }
}

// one lane: loglik = C[T-1] + ll^ in fp64, ll^ = logsumexp over the final nodes alive at the last frame of both states of the last
// normalised row (ctc_graph_score.hip's sum, in its order; a final node below the last window is stale, one above it -inf)
__global__ void ctc_graph_fb_window_loglik_kernel(int W, const int* __restrict__ fin, int n_final, const double* __restrict__ alpha_all,
                                                  const double* __restrict__ csum, const int* __restrict__ lo_of, int T,
                                                  double* __restrict__ loglik, float* __restrict__ llhat) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double2* alpha = (const double2*)alpha_all;
  const int lo_end = lo_of[T - 1];
  double m = -INFINITY;
  for (int i = 0; i < n_final; ++i) {
    if (fin[i] < lo_end || fin[i] >= lo_end + W) continue;
    const double2 v = alpha[fin[i] + 1];
    m = fmax(m, fmax(v.x, v.y));
  }
  double l = -INFINITY;
  if (m > -INFINITY) {
    double s = 0.0;
    for (int i = 0; i < n_final; ++i) {
      if (fin[i] < lo_end || fin[i] >= lo_end + W) continue;
      const double2 v = alpha[fin[i] + 1];
      s += exp(v.y - m) + exp(v.x - m);
    }
    l = m + log(s);
  }
  loglik[0] = csum[0] + l;
  llhat[0] = (float)l;
}

// per-node reductions of the posteriors, carried in HBM between launches (initialised by the host: 0, 0, -1, 0, 0)
struct GswAcc { float* occ; float* tsum; float* peak; int* peak_frame; float* visit; };

template <int NPT>
__global__ __launch_bounds__(1024) void ctc_graph_fb_window_backward_kernel(const GswSeg q, const float* __restrict__ lp, int ld, int r0,
                                                                            const int* __restrict__ rows, const int* __restrict__ node_tok,
                                                                            const int* __restrict__ soff, const unsigned* __restrict__ succs,
                                                                            const uint8_t* __restrict__ fin, int blank,
                                                                            double* __restrict__ beta_all, const float* __restrict__ cf,
                                                                            const float* __restrict__ arows, const int* __restrict__ lo_of,
                                                                            const float* __restrict__ llhat, GswAcc acc) {
  extern __shared__ __attribute__((aligned(16))) char gsw_smem[];
  double* pub = (double*)gsw_smem;                 // [2][W]: beta(T_j) of every node of the window, frames t + 1 and t
  if (q.f0 >= q.f1) return;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = q.N, W = q.W, lo = q.lo;
  const float NEG = -INFINITY;
  double2* beta = (double2*)beta_all;              // slot j + 1 = node j, as alpha
  const bool first = q.f1 == q.T;                  // this launch starts the sweep at the last frame
  const bool moved = !first && q.lo_next > lo;     // frame f1 belongs to a window further up

  unsigned col[NPT];
  unsigned arc0[NPT];                              // the node's first successor: the span j' - j | last of its list << 30 | T_j' may be entered from T_j << 31 (0: none)
  unsigned more[NPT];                              // where its further successors start (0: no such node)
  unsigned finm = 0;                               // bit k: owned node k is final
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * nth, j = lo + i;
    col[k] = (unsigned)blank * 4u; arc0[k] = 0; more[k] = 0;
    if (i < W && j < N) {
      col[k] = (unsigned)node_tok[j] * 4u;
      const int o = soff[j];
      more[k] = (unsigned)o + 1u;
      if (soff[j + 1] > o) arc0[k] = succs[o];
      if (fin[j]) finm |= 1u << k;
    }
  }

  auto row_of = [&](int fr) { return rows[max(fr, q.f0) - q.fbase] - r0; };      // below the first frame of this launch: clamped
  float eb, et[NPT];
  auto fill = [&](int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
#pragma unroll
    for (int k = 0; k < NPT; ++k) et[k] = *(const float*)(row + col[k]);
  };
  // a^(T_j) of frame fr, whose row starts at node lo_fr <= lo; -inf below frame 0 and where the node was not alive
  auto load_row = [&](float* a, int fr, int lo_fr) {
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int c = lo - lo_fr + tid + k * nth;
      a[k] = (fr >= 0 && more[k] && c < W) ? arows[(size_t)fr * W + c] : NEG;
    }
  };

  double bT[NPT], bB[NPT];
  float ac[NPT];
  float occ[NPT], ts[NPT], pk[NPT], vis[NPT];
  int pf[NPT];
  int par = 0;
  auto publish = [&]() {
    double* dst = pub + (size_t)par * W;
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      if (more[k]) dst[tid + k * nth] = bT[k];
    __syncthreads();
  };
  // The first step after a move: a node below `cut` (= lo_next) gets -inf in both states, and a successor above the window's top but
  // below `hbm_end` (= min(lo_next + W, N)) is read from beta in HBM.  After that step both are 0: no cut, above the top is -inf.
  int cut = 0, hbm_end = 0;
  // one frame.  init: frame T - 1, whose b^ is lp - ll^ in both states of the final nodes; else the recursion from the b^ of frame f + 1
  float cn = 0.f;                                  // c[f + 1] of the frame about to be computed, read one frame ahead
  auto step = [&](int f, bool init, float ll) {
    const char* rowp = (const char*)(lp + (size_t)row_of(f - 1) * ld);
    const float c = cn;
    cn = cf[f];
    const double* src = pub + (size_t)par * W;
    auto succ_b = [&](int i, unsigned arc) -> double {           // b^(T) of frame f + 1 of the successor the word names
      const int idx = i + (int)(arc & GS_SPAN);
      if (idx < W) return src[idx];
      return lo + idx < hbm_end ? beta[lo + idx + 1].x : (double)NEG;
    };
    float ap[NPT];
    load_row(ap, f - 1, f > 0 ? lo_of[f - 1] : lo);
    const float tf = (float)f;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      if (!more[k]) continue;
      const int i = tid + k * nth;
      double uT, uB;                               // log-sums over the successors' b^ of frame f + 1, before c and the emission
      if (init) {
        uT = uB = ((finm >> k) & 1u) ? -(double)ll : (double)NEG;
      } else if (arc0[k] == 0) {
        uT = dlse2(bT[k], bB[k]);
        uB = bB[k];
      } else {
        const double v0 = succ_b(i, arc0[k]);
        const double x0 = (arc0[k] & GS_T) ? v0 : (double)NEG;
        if (arc0[k] & GS_LAST) {
          uT = dlse3(bT[k], bB[k], x0);
          uB = dlse2(bB[k], v0);
        } else {
          const unsigned* sl = succs + more[k];
          double mB = fmax(bB[k], v0), mT = fmax(fmax(bT[k], bB[k]), x0);
          for (int a = 0; a < CTC_GRAPH_MAX_IN_DEGREE - 1; ++a) {
            const unsigned arc = sl[a];
            const double v = succ_b(i, arc);
            mB = fmax(mB, v);
            if (arc & GS_T) mT = fmax(mT, v);
            if (arc & GS_LAST) break;
          }
          const double mmB = mB > NEG ? mB : 0.0, mmT = mT > NEG ? mT : 0.0;
          float sB = expf((float)(bB[k] - mmB)) + expf((float)(v0 - mmB));
          float sT = expf((float)(bT[k] - mmT)) + expf((float)(bB[k] - mmT)) + expf((float)(x0 - mmT));
          for (int a = 0; a < CTC_GRAPH_MAX_IN_DEGREE - 1; ++a) {
            const unsigned arc = sl[a];
            const double v = succ_b(i, arc);
            sB += expf((float)(v - mmB));
            if (arc & GS_T) sT += expf((float)(v - mmT));
            if (arc & GS_LAST) break;
          }
          uT = mmT + (double)logf(sT);
          uB = mmB + (double)logf(sB);
        }
      }
      if (lo + i < cut) { uT = (double)NEG; uB = (double)NEG; }
      const double u = uT - (double)c;             // init: c = 0
      bT[k] = u + (double)et[k];
      bB[k] = (uB - (double)c) + (double)eb;
      const float g = expf((float)((double)ac[k] + u));            // the posterior of T_j at frame f; 0 where alpha or beta is -inf
      const float stay = expf((float)(((double)ap[k] + bT[k]) - (double)cn));   // its part that was in T_j at frame f - 1 already (0 at frame 0)
      occ[k] += g;
      ts[k] += g * tf;
      vis[k] += g - stay;
      if (g >= pk[k]) { pk[k] = g; pf[k] = f; }   // frames descend: >= keeps the first frame of a tie
      ac[k] = ap[k];
      et[k] = *(const float*)(rowp + col[k]);
    }
    eb = *(const float*)(rowp + (unsigned)blank * 4u);
    cut = 0; hbm_end = 0;
    par ^= 1;
    publish();
  };

  int f = q.f1 - 1;
  fill(row_of(f));
  load_row(ac, f, lo);
#pragma unroll
  for (int k = 0; k < NPT; ++k) {                  // the accumulators as the host has set them in HBM (0, 0, -1, 0, 0) or as the launch before left them
    const bool have = more[k] != 0;
    const int i = have ? lo + tid + k * nth : 0;
    occ[k] = have ? acc.occ[i] : 0.f;
    ts[k] = have ? acc.tsum[i] : 0.f;
    pk[k] = have ? acc.peak[i] : -1.f;
    pf[k] = have ? acc.peak_frame[i] : 0;
    vis[k] = have ? acc.visit[i] : 0.f;
  }
  if (first) {
#pragma unroll
    for (int k = 0; k < NPT; ++k) { bT[k] = NEG; bB[k] = NEG; }
    step(f, true, llhat[0]);
    --f;
  } else {
    if (moved) { cut = q.lo_next; hbm_end = min(q.lo_next + W, N); }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = lo + tid + k * nth;
      const double2 v = (more[k] && j >= cut) ? beta[j + 1] : make_double2(NEG, NEG);
      bT[k] = v.x; bB[k] = v.y;
    }
    cn = cf[q.f1];
    publish();
  }
  for (; f >= q.f0; --f) step(f, false, 0.f);

#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    if (more[k]) {
      const int j = lo + tid + k * nth;
      beta[j + 1] = make_double2(bT[k], bB[k]);
      acc.occ[j] = occ[k]; acc.tsum[j] = ts[k]; acc.peak[j] = pk[k]; acc.peak_frame[j] = pf[k]; acc.visit[j] = vis[k];
    }
  }
}

constexpr int GSW_LDS_MAX = 2 * (CTC_GRAPH_SCORE_WINDOW_MAX_NODES + 1) * (int)sizeof(double2);   // what an instantiation may be launched with
static_assert(GSW_LDS_MAX + 2 * 16 * 4 + 16 * 8 + 16 * 4 <= 160 * 1024, "the window's two rows of {T, B} in fp64 and the reductions fit one workgroup's LDS");
static_assert(CTC_GRAPH_SCORE_WINDOW_MAX_NODES <= 4096, "three instantiations: NPT = 1 / 2 / 4");

template <int NPT>
int launch_forward(hipStream_t s, int threads, size_t lds, const GswSeg& q, const float* lp, int ld, int r0, const int* rows,
                   const int* node_tok, const int* aoff, const unsigned* arcs, const unsigned* rem, int blank, double* alpha, double* csum,
                   float* coff, float* arows, int* lo_of, GswBest* best) {
  // per launch, a host call of microseconds: the attribute belongs to the current device, and engines on several devices share this code
  RVB_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_graph_fb_window_forward_kernel<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, GSW_LDS_MAX));
  ctc_graph_fb_window_forward_kernel<NPT><<<1, threads, lds, s>>>(q, lp, ld, r0, rows, node_tok, aoff, arcs, rem, blank, alpha, csum, coff, arows,
                                                                 lo_of, best);
  return OK;
}

template <int NPT>
int launch_backward(hipStream_t s, int threads, size_t lds, const GswSeg& q, const float* lp, int ld, int r0, const int* rows,
                    const int* node_tok, const int* soff, const unsigned* succs, const uint8_t* fin, int blank, double* beta, const float* coff,
                    const float* arows, const int* lo_of, const float* llhat, const GswAcc& acc) {
  RVB_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_graph_fb_window_backward_kernel<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, GSW_LDS_MAX));
  ctc_graph_fb_window_backward_kernel<NPT><<<1, threads, lds, s>>>(q, lp, ld, r0, rows, node_tok, soff, succs, fin, blank, beta, coff, arows, lo_of,
                                                                  llhat, acc);
  return OK;
}

int gsw_check(const GswSeg& q) {
  if (q.W < 64 || q.W > CTC_GRAPH_SCORE_WINDOW_MAX_NODES || q.W % 64 != 0 || q.lo < 0 || q.lo % 64 != 0 || q.lo_next < q.lo ||
      q.lo_next % 64 != 0 || q.f0 < 0 || q.f1 > q.T || q.f0 < q.fbase) {
    set_error("ctc_graph_fb_window: window out of range");
    return E_ARG;
  }
  return OK;
}

int gsw_forward(hipStream_t s, const GswSeg& q, const float* lp, int ld, int r0, const int* rows, const int* node_tok, const int* aoff,
                const unsigned* arcs, const unsigned* rem, int blank, double* alpha, double* csum, float* coff, float* arows, int* lo_of,
                GswBest* best) {
  RVB_TRY(gsw_check(q));
  const int npt = ctc_graph_npt_for(q.W), threads = ctc_threads(q.W, npt);
  const size_t lds = (size_t)2 * (q.W + 1) * sizeof(double2);
#define RVB_GSW_(NPT) RVB_TRY(launch_forward<NPT>(s, threads, lds, q, lp, ld, r0, rows, node_tok, aoff, arcs, rem, blank, alpha, csum, coff, arows, lo_of, best))
  if (npt == 1) RVB_GSW_(1);
  else if (npt == 2) RVB_GSW_(2);
  else RVB_GSW_(4);
#undef RVB_GSW_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int gsw_backward(hipStream_t s, const GswSeg& q, const float* lp, int ld, int r0, const int* rows, const int* node_tok, const int* soff,
                 const unsigned* succs, const uint8_t* fin, int blank, double* beta, const float* coff, const float* arows, const int* lo_of,
                 const float* llhat, const GswAcc& acc) {
  RVB_TRY(gsw_check(q));
  const int npt = ctc_graph_npt_for(q.W), threads = ctc_threads(q.W, npt);
  const size_t lds = (size_t)2 * q.W * sizeof(double);
#define RVB_GSW_(NPT) RVB_TRY(launch_backward<NPT>(s, threads, lds, q, lp, ld, r0, rows, node_tok, soff, succs, fin, blank, beta, coff, arows, lo_of, llhat, acc))
  if (npt == 1) RVB_GSW_(1);
  else if (npt == 2) RVB_GSW_(2);
  else RVB_GSW_(4);
#undef RVB_GSW_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int pad64(int v) { return (v + 63) / 64 * 64; }

int fill32(hipStream_t s, void* p, float v, size_t n) {
  int bits;
  memcpy(&bits, &v, 4);
  RVB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)p, bits, n, s));
  return OK;
}

// n doubles of -inf
__global__ void gsw_fill_neg_kernel(double* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = -INFINITY;
}
int fill_neg64(hipStream_t s, void* p, size_t n) {
  gsw_fill_neg_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((double*)p, n);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

const char* const WHO = "ctc score graph long";

}  // namespace

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcGraphWindowScorer::plan(const char* who, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                               const uint8_t* is_final, int64_t total_frames, int window_nodes, int V, int blank_id, bool posteriors) {
  const std::string w(who), at = w + ": ";
  open = false;
  if (window_nodes != 0 && (window_nodes < 256 || window_nodes > CTC_GRAPH_SCORE_WINDOW_MAX_NODES || window_nodes % 256 != 0)) {
    set_error(at + "window_nodes " + std::to_string(window_nodes) + " must be 0 (the default, " +
              std::to_string(CTC_GRAPH_SCORE_WINDOW_DEFAULT_NODES) + ") or a multiple of 256 in [256, " +
              std::to_string(CTC_GRAPH_SCORE_WINDOW_MAX_NODES) + "]");
    return E_ARG;
  }
  CtcGraphWindowAligner p;                         // its checks and words, its arc words and the policy's tables
  RVB_TRY(p.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, total_frames,
                 window_nodes ? window_nodes : (int)CTC_GRAPH_SCORE_WINDOW_DEFAULT_NODES, V, blank_id, 0.f));
  const int N_ = p.N;
  const int32_t* y = node_tokens;
  for (int j = 0; j < N_; ++j)
    if (y[j] == RVB_CTC_WILDCARD) {
      set_error(at + "node " + std::to_string(j) + ": a wildcard has no full-sum score (the maximum over the vocabulary is no probability)");
      return E_ARG;
    }
  // The fewest frames from T_j / B_j to a final end: T_j's is the need[] of CtcGraphWindowAligner::plan (a successor of the same label
  // costs one frame more, for the blank between), B_j's one more than the nearest successor's.  Successors come later in the order,
  // so one descending pass settles them.  Beside it the out-degrees, for the transposed arcs.
  std::vector<uint32_t> remT((size_t)N_, GS_FAR), remB((size_t)N_, GS_FAR);
  std::vector<int32_t> out_deg((size_t)N_ + 1, 0);
  uint32_t rem_start = GS_FAR;
  for (int j = N_ - 1; j >= 0; --j) {
    if (is_final[j]) remT[j] = remB[j] = 0;
    for (int a = pred_off[j]; a < pred_off[j + 1]; ++a) {
      const int pr = preds[a];
      if (pr >= 0) ++out_deg[pr];
      if (remT[j] >= GS_FAR) continue;
      if (pr < 0) { rem_start = std::min(rem_start, remT[j] + 1); continue; }
      remT[pr] = std::min(remT[pr], remT[j] + (y[pr] != y[j] ? 1u : 2u));
      remB[pr] = std::min(remB[pr], remT[j] + 1);
    }
  }
  if (posteriors)
    for (int j = 0; j < N_; ++j)
      if (out_deg[j] > CTC_GRAPH_MAX_IN_DEGREE) {
        set_error(at + "node " + std::to_string(j) + ": out-degree " + std::to_string(out_deg[j]) + " exceeds the cap of " +
                  std::to_string(CTC_GRAPH_MAX_IN_DEGREE) + " successors per node (posteriors sweep the graph backwards)");
        return E_UNSUPPORTED;
      }
  h_rem.clear();
  h_rem.reserve(2 * (size_t)N_ + 1);
  for (int j = 0; j < N_; ++j) { h_rem.push_back(remT[j]); h_rem.push_back(remB[j]); }
  h_rem.push_back(rem_start);
  // the transposed arcs: per node its successors, ascending, as words relative to the node
  h_succ_off.assign((size_t)N_ + 1, 0);
  for (int j = 0; j < N_; ++j) h_succ_off[j + 1] = h_succ_off[j] + out_deg[j];
  h_succs.assign((size_t)std::max(h_succ_off[N_], 1), 0u);
  std::vector<int32_t> fillp(h_succ_off.begin(), h_succ_off.begin() + N_);
  for (int j = 0; j < N_; ++j)
    for (int a = pred_off[j]; a < pred_off[j + 1]; ++a) {
      const int pr = preds[a];
      if (pr < 0) continue;
      const int at_ = fillp[pr]++;
      h_succs[at_] = (uint32_t)(j - pr) | (y[pr] != y[j] ? GS_T : 0u) | (at_ + 1 == h_succ_off[pr + 1] ? GS_LAST : 0u);
    }
  h_fin.assign(is_final, is_final + N_);
  N = N_; T = p.T; W = p.W; blank = p.blank;
  tab = p.tab;
  h_tokens.swap(p.h_tokens); h_arc_off.swap(p.h_arc_off); h_arcs.swap(p.h_arcs); h_finals.swap(p.h_finals);
  row_bytes = (size_t)T * (size_t)W * 4;
  post = posteriors;
  h_rows.clear(); launches.clear(); batches.clear();
  fed = fbase = 0; lo = 0; best = -1; back = 0; back_batch = 0; cursor = 0;
  forward_done = false;
  lo_force = nullptr; n_force = 0;
  return OK;
}

int CtcGraphWindowScorer::begin(hipStream_t s) {
  RVB_TRY(d_tokens.ensure((size_t)N * 4));
  RVB_TRY(d_arc_off.ensure(((size_t)N + 1) * 4));
  RVB_TRY(d_arcs.ensure(h_arcs.size() * 4));
  RVB_TRY(d_finals.ensure(h_finals.size() * 4));
  RVB_TRY(d_rem.ensure(h_rem.size() * 4));
  RVB_TRY(d_alpha.ensure(((size_t)N + 1) * 16));
  RVB_TRY(d_lo.ensure((size_t)T * 4));
  RVB_TRY(d_csum.ensure(8));
  RVB_TRY(d_loglik.ensure(8));
  RVB_TRY(d_llhat.ensure(4));
  RVB_TRY(d_best.ensure(sizeof(GswBest)));
  if (post) {
    if (int r = d_arows.ensure(row_bytes)) {
      set_error(std::string(WHO) + ": " + std::to_string(row_bytes) + " bytes of alpha rows (4 bytes per frame and window node) do not fit: " +
                last_error());
      return r;
    }
    RVB_TRY(d_coff.ensure((size_t)T * 4));
    RVB_TRY(d_beta.ensure(((size_t)N + 1) * 16));
    RVB_TRY(d_acc.ensure((size_t)N * 20));
    RVB_TRY(d_succ_off.ensure(h_succ_off.size() * 4));
    RVB_TRY(d_succs.ensure(h_succs.size() * 4));
    RVB_TRY(d_fin.ensure(h_fin.size()));
    RVB_HIP_CHECK(hipMemcpyAsync(d_succ_off.p, h_succ_off.data(), h_succ_off.size() * 4, hipMemcpyHostToDevice, s));
    RVB_HIP_CHECK(hipMemcpyAsync(d_succs.p, h_succs.data(), h_succs.size() * 4, hipMemcpyHostToDevice, s));
    RVB_HIP_CHECK(hipMemcpyAsync(d_fin.p, h_fin.data(), h_fin.size(), hipMemcpyHostToDevice, s));
    float* acc = d_acc.as<float>();
    RVB_TRY(fill_neg64(s, d_beta.p, ((size_t)N + 1) * 2));
    RVB_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)N * 20, s));        // occupancy, frame-weighted sum, peak frame, visit: 0
    RVB_TRY(fill32(s, acc + 2 * (size_t)N, -1.f, (size_t)N));        // peak posterior: below every posterior
  }
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_arc_off.p, h_arc_off.data(), ((size_t)N + 1) * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_arcs.p, h_arcs.data(), h_arcs.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_finals.p, h_finals.data(), h_finals.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_rem.p, h_rem.data(), h_rem.size() * 4, hipMemcpyHostToDevice, s));
  RVB_TRY(fill_neg64(s, d_alpha.p, ((size_t)N + 1) * 2));
  RVB_HIP_CHECK(hipMemsetAsync(d_csum.p, 0, 8, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));          // the host vectors may be replaced by the next plan()
  open = true;
  return OK;
}

int CtcGraphWindowScorer::batch(hipStream_t s, const std::vector<int32_t>& rows) {
  if (!open) { set_error(std::string(WHO) + ": feed before begin"); return E_STATE; }
  if (forward_done) { set_error(std::string(WHO) + ": feed after the forward sweep was finished"); return E_STATE; }
  if (fed != fbase + (int64_t)h_rows.size()) { set_error(std::string(WHO) + ": the slabs did not cover every frame of the batch before"); return E_STATE; }
  if (fed + (int64_t)rows.size() > T) {
    set_error(std::string(WHO) + ": feed after the lattice's frames are used up: " + std::to_string(fed) + " of " + std::to_string(T) +
              " frames fed, the batch holds " + std::to_string(rows.size()) + " more");
    return E_STATE;
  }
  for (size_t f = 1; f < rows.size(); ++f)
    if (rows[f] <= rows[f - 1]) { set_error(std::string(WHO) + ": frame rows must increase"); return E_ARG; }
  h_rows = rows;
  fbase = fed;
  batches.push_back((int)rows.size());
  RVB_TRY(d_rows.ensure(std::max<size_t>(rows.size(), 1) * 4));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  RVB_HIP_CHECK(hipMemcpy(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice));
  return OK;
}

bool CtcGraphWindowScorer::touches(int r0, int nrows) const {
  const auto a = std::lower_bound(h_rows.begin(), h_rows.end(), r0), b = std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows);
  return a != b;
}

int CtcGraphWindowScorer::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  if (!open) { set_error(std::string(WHO) + ": feed before begin"); return E_STATE; }
  if (forward_done) { set_error(std::string(WHO) + ": feed after the forward sweep was finished"); return E_STATE; }
  const int b0 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0) - h_rows.begin());
  const int b1 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows) - h_rows.begin());
  if (b0 == b1) return OK;
  if (fbase + b0 != fed) { set_error(std::string(WHO) + ": slabs must arrive in row order"); return E_STATE; }
  for (int g0 = fbase + b0, end = fbase + b1; g0 < end;) {
    int g1;
    if (lo_force) {                                // lab hook: a slab is one launch, in the window given for it
      if ((int)launches.size() >= n_force) { set_error(std::string(WHO) + ": more launches than forced windows"); return E_STATE; }
      lo = lo_force[launches.size()]; g1 = end;
    } else {
      const CtcGraphWindowStep st = ctc_graph_window_next(tab, T, W, g0, end, lo, best);
      lo = st.lo; g1 = st.f1;
    }
    if (g1 <= g0 || g1 > end || lo < 0 || lo % 64 != 0 || lo > std::max(0, pad64(N) - W) || (g0 == 0 && lo != 0)) {
      set_error(std::string(WHO) + ": the window policy left its bounds");
      return E_HIP;
    }
    GswSeg q{N, T, W, lo, lo, g0, g1, fbase};
    RVB_TRY(gsw_forward(s, q, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), d_arc_off.as<int>(), d_arcs.as<unsigned>(), d_rem.as<unsigned>(),
                        blank, d_alpha.as<double>(), d_csum.as<double>(), post ? d_coff.as<float>() : nullptr,
                        post ? d_arows.as<float>() : nullptr, d_lo.as<int>(), d_best.as<GswBest>()));
    GswBest hb;
    RVB_HIP_CHECK(hipMemcpyAsync(&hb, d_best.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    RVB_HIP_CHECK(hipStreamSynchronize(s));        // the one synchronisation of a launch: the next window depends on it
    best = hb.node;
    launches.push_back({g0, g1, lo, best});
    fed = g1;
    g0 = g1;
  }
  return OK;
}

int CtcGraphWindowScorer::loglik(hipStream_t s, double* loglik_out) {
  if (!open) { set_error(std::string(WHO) + ": loglik before begin"); return E_STATE; }
  if (fed != T) {
    set_error(std::string(WHO) + ": loglik before all " + std::to_string(T) + " frames were fed (" + std::to_string(fed) + " so far)");
    return E_STATE;
  }
  double ll = 0.0;
  ctc_graph_fb_window_loglik_kernel<<<1, 64, 0, s>>>(W, d_finals.as<int>(), (int)h_finals.size(), d_alpha.as<double>(), d_csum.as<double>(),
                                                     d_lo.as<int>(), T, d_loglik.as<double>(), d_llhat.as<float>());
  RVB_HIP_CHECK(hipGetLastError());
  RVB_HIP_CHECK(hipMemcpyAsync(&ll, d_loglik.p, 8, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  if (!(ll > -INFINITY)) {
    set_error(std::string(WHO) + ": infeasible: no path inside the window of " + std::to_string(W) + " nodes ends in a final node after " +
              std::to_string(T) + " frames with a finite score");
    return E_ARG;
  }
  if (!forward_done) {                             // the backward sweep starts above the last frame, at the last batch and launch
    forward_done = true;
    back = T;
    back_batch = (int)batches.size();
    cursor = (int)launches.size();
    h_rows.clear();
    fbase = T;
  }
  if (loglik_out) *loglik_out = ll;
  return OK;
}

int CtcGraphWindowScorer::batch_back(hipStream_t s, const std::vector<int32_t>& rows) {
  if (!open) { set_error(std::string(WHO) + ": feed before begin"); return E_STATE; }
  if (!post) { set_error(std::string(WHO) + ": backward sweep without alpha rows"); return E_STATE; }
  if (!forward_done) { set_error(std::string(WHO) + ": the backward sweep starts after the forward sweep was finished"); return E_STATE; }
  if (back != fbase) { set_error(std::string(WHO) + ": the slabs did not cover every frame of the batch before"); return E_STATE; }
  if (back_batch <= 0) { set_error(std::string(WHO) + ": the backward sweep has reached the first frame: no batch is left"); return E_STATE; }
  const int want = batches[back_batch - 1];
  if ((int)rows.size() != want) {
    set_error(std::string(WHO) + ": the backward sweep takes the batches in descending order: expected batch " + std::to_string(back_batch - 1) +
              " with the " + std::to_string(want) + " frames [" + std::to_string(back - want) + ", " + std::to_string(back) +
              ") of the forward sweep, got " + std::to_string(rows.size()) + " frames");
    return E_STATE;
  }
  for (size_t f = 1; f < rows.size(); ++f)
    if (rows[f] <= rows[f - 1]) { set_error(std::string(WHO) + ": frame rows must increase"); return E_ARG; }
  h_rows = rows;
  --back_batch;
  fbase = back - want;
  RVB_TRY(d_rows.ensure(std::max<size_t>(rows.size(), 1) * 4));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  RVB_HIP_CHECK(hipMemcpy(d_rows.p, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice));
  return OK;
}

int CtcGraphWindowScorer::advance_back(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  if (!open) { set_error(std::string(WHO) + ": feed before begin"); return E_STATE; }
  if (!post) { set_error(std::string(WHO) + ": backward sweep without alpha rows"); return E_STATE; }
  if (!forward_done) { set_error(std::string(WHO) + ": the backward sweep starts after the forward sweep was finished"); return E_STATE; }
  const int b0 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0) - h_rows.begin());
  const int b1 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows) - h_rows.begin());
  if (b0 == b1) return OK;
  if (fbase + b1 != back) { set_error(std::string(WHO) + ": the backward sweep takes the slabs in descending row order"); return E_STATE; }
  float* acc = d_acc.as<float>();
  const size_t n = (size_t)N;
  const GswAcc a{acc, acc + n, acc + 2 * n, (int*)(acc + 3 * n), acc + 4 * n};
  // the recorded launches that hold the slab's frames, last first, each with its own window; one that the slab holds only in part is
  // run in part, which changes nothing: beta and the accumulators are carried exactly
  for (const int low = fbase + b0; back > low;) {
    while (cursor > 0 && launches[cursor - 1].f0 >= back) --cursor;
    const Launch& m = launches[cursor - 1];
    const int g1 = back, g0 = std::max(m.f0, low);
    const int lo_next = g1 == m.f1 && cursor < (int)launches.size() ? launches[cursor].lo : m.lo;
    GswSeg q{N, T, W, m.lo, lo_next, g0, g1, fbase};
    RVB_TRY(gsw_backward(s, q, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), d_succ_off.as<int>(), d_succs.as<unsigned>(),
                         d_fin.as<uint8_t>(), blank, d_beta.as<double>(), d_coff.as<float>(), d_arows.as<float>(), d_lo.as<int>(),
                         d_llhat.as<float>(), a));
    back = g0;
  }
  return OK;
}

int CtcGraphWindowScorer::finish(hipStream_t s, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  if (!open) { set_error(std::string(WHO) + ": finish before begin"); return E_STATE; }
  if (!post) { set_error(std::string(WHO) + ": backward sweep without alpha rows"); return E_STATE; }
  if (!forward_done || back != 0) {
    set_error(std::string(WHO) + ": the backward sweep did not reach the first frame (" + std::to_string(forward_done ? back : T) +
              " frames to go)");
    return E_STATE;
  }
  const size_t n = (size_t)N;
  std::vector<float> h(5 * n);
  RVB_HIP_CHECK(hipMemcpyAsync(h.data(), d_acc.p, n * 20, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  for (size_t k = 0; k < n; ++k) {
    if (occupancy) occupancy[k] = h[k];
    if (mean_frame) mean_frame[k] = h[k] > 0.f ? h[n + k] / h[k] : -1.f;      // no mass at all: no frame
    if (peak_post) peak_post[k] = h[2 * n + k];
    if (visit) visit[k] = h[4 * n + k];
  }
  if (peak_frame) memcpy(peak_frame, h.data() + 3 * n, n * 4);
  return OK;
}

void CtcGraphWindowScorer::release() {
  for (DevBuf* b : {&d_tokens, &d_arc_off, &d_arcs, &d_finals, &d_rows, &d_rem, &d_alpha, &d_lo, &d_csum, &d_loglik, &d_llhat, &d_best, &d_coff,
                    &d_arows, &d_beta, &d_acc, &d_succ_off, &d_succs, &d_fin})
    b->release();
  open = false;
}

}  // namespace rvb
