// CTC full-sum scoring over a left-to-right token GRAPH (alternatives and optional words): the log-semiring sibling of ctc_graph.hip,
// with the normalised log-sum-exp sweeps of ctc_forward_backward.hip.  Graph, labels, predecessor lists, finals and states (B_start,
// per node T_j and B_j) are those of ctc_graph.hip; no wildcards (max_v lp is no probability).
//
//   frame 0:  a(B_start) = lp[0][blank];  a(T_j) = lp[0][tok_j] if -1 is in pred[j], else -inf;  a(B_j) = -inf
//   frame t:  a(B_start) = a'(B_start) + lp[t][blank]
//             a(B_j)     = lse(a'(B_j), a'(T_j)) + lp[t][blank]
//             a(T_j)     = lse(a'(T_j), per predecessor p: a'(B_p) (a'(B_start) for -1), a'(T_p) if tok_p != tok_j) + lp[t][tok_j]
//   loglik   = lse over the final nodes f of a_{T-1}(B_f), a_{T-1}(T_f)
//   beta is the mirror image over the successors and includes the emission of its own frame;
//   gamma_t(T_j) = a_t(T_j) + beta_t(T_j) - lp[t][tok_j] - loglik
//
// Every (node path, CTC alignment of its labels) pair is exactly one state path, so loglik = log sum over node paths pi of
// p_CTC(labels(pi) | frames).  Two node paths that spell the same tokens are two paths: {a|a} scores loglik(a) + log 2.
//
// Normalisation, as in ctc_forward_backward.hip: the kernels carry a^[t] = alpha[t] - C[t], C[t] = c[1] + ... + c[t], c[t] an fp32
// value subtracted as it is and summed in fp64 by thread 0.  Unlike there, a^ and b^ themselves are fp64 (see dlse3 below); only the
// stored rows a^(T_j) are fp32, rounded once where they are written.  c[t] is the maximum of the row a^[t-1] over the states that can still
// reach the end: the host computes per node the fewest frames from T_j (and from B_j) to a final end (a successor of the same label
// costs one frame more, for the blank between), and a state counts while that is within the frames left.  The maximum is reduced
// inside each wave, published before the one barrier of its frame and combined by every thread after it.  The backward sweep carries
// b^[t] = beta[t] - (loglik - C[t]), so exp(a^ + b^ - lp) is the posterior with no scalar left over.
//
// Shape: that of ctc_graph.hip.  ONE workgroup per lattice, one __syncthreads() per frame, thread tid owns nodes tid, tid + nthreads,
// ... (NPT = 1 / 2 / 4 / 8), {T, B} of every slot published in the LDS array, 16 bytes per slot: double-buffered up to 5087 nodes, and
// above that ONE buffer of 128 KiB with a second barrier per frame between the reads and the writes (the backward sweep publishes T
// alone, a successor's blank is never entered from outside: two buffers of 64 KiB at the cap, one barrier), the first arc of each node in a register, the further ones read through the L1,
// the next frame's emissions gathered before the barrier, alpha (beta) in HBM between slabs.  With posteriors the forward sweep
// stores a^(T_j) of every frame (4 bytes per frame and node, N padded to 64) and its offsets; the backward kernel, over the
// host-built transposed arc list, reads the rows of frames t and t - 1 and reduces occupancy, the frame-weighted sum, the peak
// posterior with its frame and the visit probability in registers of the thread that owns the node: no atomics.
//   visit_j = sum_t [exp(gamma_t(T_j)) - exp(a_{t-1}(T_j) + beta_t(T_j) - loglik)]     (the mass that ENTERS T_j at frame t)
// A cell whose predecessors are all -inf stays -inf (the maximum is replaced by 0 before it is subtracted): no NaN.  Every loop is
// bounded by T, a node count or a degree.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace rvb {

namespace {

constexpr unsigned REM_NEVER = 0xffffu;                   // frames to the end of a state that reaches no final node

// The states are CARRIED in fp64 (registers, LDS, HBM between slabs): the state that carries the posterior may lie hundreds of nats
// below the row maximum the normaliser follows, and an fp32 cell would round it at that magnitude once per frame in each sweep, an
// error common to a row that only a division by the row's summed posterior could remove.  The transcendental part stays fp32: the
// differences to the maximum are exact in fp64, rounded to fp32 (magnitude <= ~88 where they matter), and log of the sum is a small
// fp32 number added to the fp64 maximum.
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
__global__ __launch_bounds__(1024) void ctc_graph_sum_forward_kernel(const GraphSeq* __restrict__ seqs, const float* __restrict__ lp, int ld,
                                                                     int r0, const int* __restrict__ rows, const int* __restrict__ node_tok,
                                                                     const int* __restrict__ arc_off_all, const unsigned* __restrict__ arcs_all,
                                                                     const unsigned* __restrict__ rem_all, int blank,
                                                                     double* __restrict__ alpha_all, double* __restrict__ csum,
                                                                     float* __restrict__ coff, float* __restrict__ arows, int slots_cap,
                                                                     int single) {
  extern __shared__ __attribute__((aligned(16))) char cgs_smem[];
  // [2][slots_cap]: {T, B} of every slot, frames t - 1 and t.  single: ONE buffer (above 5087 nodes two do not fit the LDS): the
  // frame's reads end at a barrier of their own before the row is overwritten
  double2* pub = (double2*)cgs_smem;
  __shared__ float wmx[2][16];                     // per wave: maximum of the row over the live states
  const GraphSeq q = seqs[blockIdx.x];
  if (q.f0 >= q.f1) return;                        // nothing of this lattice in the slab (uniform over the workgroup)
  const int tid = threadIdx.x, nth = blockDim.x, nw = nth >> 6;
  const int N = q.N;
  const float NEG = -INFINITY;
  const int* rw = rows + q.frame_off;
  const int* aoff = arc_off_all + q.node_off + q.index;        // N + 1 offsets per lattice
  const unsigned* arcs = arcs_all + q.arc_off;
  const unsigned* rem = rem_all + q.node_off + q.index;         // N + 1 words per lattice, the last one B_start's
  double2* alpha = (double2*)(alpha_all + q.alpha_off);         // [N + 1] slots
  float* arow = arows ? arows + q.bp_off : nullptr;             // the T rows share the layout of the aligner's back-pointers, in floats

  unsigned col[NPT];                               // byte offset of the node's column in a row of lp
  unsigned arc0[NPT];                              // the node's first arc
  unsigned meta[NPT];                              // where its further arcs start | its in-degree << 16 (0: no such node)
  unsigned rm[NPT];                                // frames to the end from T_j | from B_j << 16
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = tid + k * nth;
    col[k] = (unsigned)blank * 4u; arc0[k] = 0; meta[k] = 0; rm[k] = REM_NEVER | REM_NEVER << 16;
    if (j < N) {
      col[k] = (unsigned)node_tok[q.node_off + j] * 4u;
      const int o = aoff[j];
      meta[k] = (unsigned)(o + 1) | (unsigned)(aoff[j + 1] - o) << 16; arc0[k] = arcs[o];
      rm[k] = rem[j];
    }
  }
  const unsigned rem_start = rem[N] & 0xffffu;

  auto row_of = [&](int fr) { return rw[min(fr, q.f1 - 1)] - r0; };   // past the launch's last frame: clamped, a harmless in-bounds load
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
    if (single) __syncthreads();
    double2* dst = pub + (size_t)par * slots_cap;
    const unsigned left = (unsigned)min(q.T - 1 - fr, (int)REM_NEVER - 1);
    float m = NEG;
    if (tid == 0) { dst[0] = make_double2(NEG, bstart); if (rem_start <= left) m = (float)bstart; }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      if (j < N) {
        dst[j + 1] = make_double2(aT[k], aB[k]);
        m = fmaxf(m, (rm[k] & 0xffffu) <= left ? (float)aT[k] : NEG);
        m = fmaxf(m, (rm[k] >> 16) <= left ? (float)aB[k] : NEG);
      }
    }
    m = wave_max(m);
    if ((tid & 63) == 0) wmx[par][tid >> 6] = m;
    __syncthreads();
  };
  auto store_row = [&](int fr) {
    if (!arow) return;
    float* dst = arow + (size_t)fr * q.bp_stride;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      if (j < N) dst[j] = (float)aT[k];
    }
  };

  int f = q.f0;
  double C = 0.0;
  fill(row_of(f));
  if (f == 0) {
    bstart = eb;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      // -1 among the predecessors: bounded by the in-degree (frame 0 only)
      bool from_start = false;
      const int deg = (int)(meta[k] >> 16), a1 = (int)(meta[k] & 0xffffu);
      for (int a = 0; a < deg; ++a) from_start = from_start || ((a == 0 ? arc0[k] : arcs[a1 + a - 1]) & ARC_SLOT) == 0;
      aT[k] = from_start ? et[k] : NEG;
      aB[k] = NEG;
    }
    if (tid == 0 && coff) coff[q.frame_off] = 0.f;
    store_row(0);
    f = 1;
    fill(row_of(1));
  } else {
    bstart = alpha[0].y;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      const double2 v = j < N ? alpha[j + 1] : make_double2(NEG, NEG);
      aT[k] = v.x; aB[k] = v.y;
    }
    if (tid == 0) C = csum[blockIdx.x];
  }
  publish(f - 1);

  for (; f < q.f1; ++f) {
    const char* rown = (const char*)(lp + (size_t)row_of(f + 1) * ld);   // frame f + 1's emissions: loaded as this frame's are used up
    const double2* src = pub + (size_t)par * slots_cap;
    float m = wmx[par][0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, wmx[par][w]);
    const float c = m > NEG ? m : 0.f;             // the offset of this frame: the maximum of the row before it
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int deg = (int)(meta[k] >> 16), a1 = (int)(meta[k] & 0xffffu);
      if (deg > 0) {
        const double2 v0 = src[arc0[k] & ARC_SLOT];
        const double x1 = v0.y, x2 = (arc0[k] & ARC_T) ? v0.x : (double)NEG;
        double t;
        if (deg == 1) {
          t = dlse3(aT[k], x1, x2);
        } else {
          double mx = fmax(aT[k], fmax(x1, x2));
          for (int a = 1; a < deg; ++a) {
            const unsigned arc = arcs[a1 + a - 1];
            const double2 v = src[arc & ARC_SLOT];
            mx = fmax(mx, fmax(v.y, (arc & ARC_T) ? v.x : (double)NEG));
          }
          const double mm = mx > NEG ? mx : 0.0;
          float s = expf((float)(aT[k] - mm)) + expf((float)(x1 - mm)) + expf((float)(x2 - mm));
          for (int a = 1; a < deg; ++a) {
            const unsigned arc = arcs[a1 + a - 1];
            const double2 v = src[arc & ARC_SLOT];
            s += expf((float)(v.y - mm));
            if (arc & ARC_T) s += expf((float)(v.x - mm));
          }
          t = mm + (double)logf(s);
        }
        aB[k] = (dlse2(aB[k], aT[k]) + (double)eb) - (double)c;
        aT[k] = (t + (double)et[k]) - (double)c;
        et[k] = *(const float*)(rown + col[k]);
      }
    }
    bstart = (bstart + (double)eb) - (double)c;
    eb = *(const float*)(rown + (unsigned)blank * 4u);
    if (tid == 0) { C += (double)c; if (coff) coff[q.frame_off + f] = c; }
    store_row(f);
    if (!single) par ^= 1;
    publish(f);
  }
  if (tid == 0) { alpha[0] = make_double2(NEG, bstart); csum[blockIdx.x] = C; }
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = tid + k * nth;
    if (j < N) alpha[j + 1] = make_double2(aT[k], aB[k]);
  }
}

// one lane per lattice: loglik = C[T-1] + ll^ in fp64, ll^ = logsumexp over the final nodes of both states of the last normalised row
__global__ void ctc_graph_sum_loglik_kernel(const GraphSeq* __restrict__ seqs, const int* __restrict__ finals_all,
                                            const double* __restrict__ alpha_all, const double* __restrict__ csum, double* __restrict__ loglik,
                                            float* __restrict__ llhat) {
  if (threadIdx.x != 0) return;
  const GraphSeq q = seqs[blockIdx.x];
  const double2* alpha = (const double2*)(alpha_all + q.alpha_off);
  const int* fin = finals_all + q.fin_off;
  double m = -INFINITY;
  for (int i = 0; i < q.n_final; ++i) {
    const double2 v = alpha[fin[i] + 1];
    m = fmax(m, fmax(v.x, v.y));
  }
  double l = -INFINITY;
  if (m > -INFINITY) {
    double s = 0.0;
    for (int i = 0; i < q.n_final; ++i) {
      const double2 v = alpha[fin[i] + 1];
      s += exp(v.y - m) + exp(v.x - m);
    }
    l = m + log(s);
  }
  loglik[blockIdx.x] = csum[blockIdx.x] + l;
  llhat[blockIdx.x] = (float)l;
}

// per-node reductions of the posteriors, carried in HBM between launches
struct GsAcc { float* occ; float* tsum; float* peak; int* peak_frame; float* visit; };

template <int NPT>
__global__ __launch_bounds__(1024) void ctc_graph_sum_backward_kernel(const GraphSeq* __restrict__ seqs, const float* __restrict__ lp, int ld,
                                                                      int r0, const int* __restrict__ rows, const int* __restrict__ node_tok,
                                                                      const int* __restrict__ succ_off_all,
                                                                      const unsigned* __restrict__ succs_all, const uint8_t* __restrict__ fin_all,
                                                                      int blank, double* __restrict__ beta_all, const float* __restrict__ coff,
                                                                      const float* __restrict__ arows, const float* __restrict__ llhat,
                                                                      GsAcc acc, int slots_cap) {
  extern __shared__ __attribute__((aligned(16))) char cgs_smem[];
  double* pub = (double*)cgs_smem;                 // [2][slots_cap]: beta(T_j) of every node, frames t + 1 and t (128 KiB at the cap)
  const GraphSeq q = seqs[blockIdx.x];
  if (q.f0 >= q.f1) return;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = q.N;
  const float NEG = -INFINITY;
  const int* rw = rows + q.frame_off;
  const int* soff = succ_off_all + q.node_off + q.index;        // N + 1 offsets per lattice
  const unsigned* succs = succs_all + q.arc_off;
  double2* beta = (double2*)(beta_all + q.alpha_off);           // slot j + 1 = node j, as alpha
  const float* cf = coff + q.frame_off;
  const float* arow = arows + q.bp_off;
  const bool first = q.f1 == q.T;                  // this launch starts the sweep at the last frame

  unsigned col[NPT];
  unsigned arc0[NPT];                              // the node's first successor: node | its T may be entered from T_j << 15
  unsigned meta[NPT];                              // where its further successors start | out-degree << 16 | owned << 30 | final << 31
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = tid + k * nth;
    col[k] = (unsigned)blank * 4u; arc0[k] = 0; meta[k] = 0;
    if (j < N) {
      col[k] = (unsigned)node_tok[q.node_off + j] * 4u;
      const int o = soff[j], deg = soff[j + 1] - o;
      meta[k] = (unsigned)(o + 1) | (unsigned)deg << 16 | 1u << 30 | (fin_all[q.node_off + j] ? 1u << 31 : 0u);
      if (deg > 0) arc0[k] = succs[o];
    }
  }

  auto row_of = [&](int fr) { return rw[max(fr, q.f0)] - r0; };      // below the first frame of this launch: clamped
  float eb, et[NPT];
  auto fill = [&](int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
#pragma unroll
    for (int k = 0; k < NPT; ++k) et[k] = *(const float*)(row + col[k]);
  };
  auto load_row = [&](float* a, int fr) {          // a^(T_j) of frame fr; -inf below frame 0
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      a[k] = (fr >= 0 && j < N) ? arow[(size_t)fr * q.bp_stride + j] : NEG;
    }
  };

  double bT[NPT], bB[NPT];
  float ac[NPT];
  float occ[NPT], ts[NPT], pk[NPT], vis[NPT];
  int pf[NPT];
  int par = 0;
  auto publish = [&]() {
    double* dst = pub + (size_t)par * slots_cap;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      if (j < N) dst[j] = bT[k];
    }
    __syncthreads();
  };
  // one frame.  init: frame T - 1, whose b^ is lp - ll^ in both states of the final nodes; else the recursion from the b^ of frame f + 1
  float cn = 0.f;                                  // c[f + 1] of the frame about to be computed, read one frame ahead
  auto step = [&](int f, bool init, float ll) {
    const char* rowp = (const char*)(lp + (size_t)row_of(f - 1) * ld);
    const float c = cn;
    cn = cf[f];
    const double* src = pub + (size_t)par * slots_cap;
    float ap[NPT];
    load_row(ap, f - 1);
    const float tf = (float)f;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      if (!(meta[k] >> 30 & 1u)) continue;
      const int deg = (int)(meta[k] >> 16 & 0x7fu), a1 = (int)(meta[k] & 0xffffu);
      double uT, uB;                             // log-sums over the successors' b^ of frame f + 1, before c and the emission
      if (init) {
        uT = uB = (meta[k] >> 31) ? -(double)ll : (double)NEG;
      } else if (deg == 0) {
        uT = dlse2(bT[k], bB[k]);
        uB = bB[k];
      } else {
        const double v0 = src[arc0[k] & ARC_SLOT];
        const double x0 = (arc0[k] & ARC_T) ? v0 : (double)NEG;
        if (deg == 1) {
          uT = dlse3(bT[k], bB[k], x0);
          uB = dlse2(bB[k], v0);
        } else {
          double mB = fmax(bB[k], v0), mT = fmax(fmax(bT[k], bB[k]), x0);
          for (int a = 1; a < deg; ++a) {
            const unsigned arc = succs[a1 + a - 1];
            const double v = src[arc & ARC_SLOT];
            mB = fmax(mB, v);
            if (arc & ARC_T) mT = fmax(mT, v);
          }
          const double mmB = mB > NEG ? mB : 0.0, mmT = mT > NEG ? mT : 0.0;
          float sB = expf((float)(bB[k] - mmB)) + expf((float)(v0 - mmB));
          float sT = expf((float)(bT[k] - mmT)) + expf((float)(bB[k] - mmT)) + expf((float)(x0 - mmT));
          for (int a = 1; a < deg; ++a) {
            const unsigned arc = succs[a1 + a - 1];
            const double v = src[arc & ARC_SLOT];
            sB += expf((float)(v - mmB));
            if (arc & ARC_T) sT += expf((float)(v - mmT));
          }
          uT = mmT + (double)logf(sT);
          uB = mmB + (double)logf(sB);
        }
      }
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
    par ^= 1;
    publish();
  };

  int f = q.f1 - 1;
  fill(row_of(f));
  load_row(ac, f);
  if (first) {
#pragma unroll
    for (int k = 0; k < NPT; ++k) { occ[k] = 0.f; ts[k] = 0.f; pk[k] = -1.f; pf[k] = 0; vis[k] = 0.f; bT[k] = NEG; bB[k] = NEG; }
    step(f, true, llhat[blockIdx.x]);
    --f;
  } else {
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int j = tid + k * nth;
      const bool have = j < N;
      const double2 v = have ? beta[j + 1] : make_double2(NEG, NEG);
      bT[k] = v.x; bB[k] = v.y;
      const int i = q.node_off + (have ? j : 0);
      occ[k] = have ? acc.occ[i] : 0.f;
      ts[k] = have ? acc.tsum[i] : 0.f;
      pk[k] = have ? acc.peak[i] : -1.f;
      pf[k] = have ? acc.peak_frame[i] : 0;
      vis[k] = have ? acc.visit[i] : 0.f;
    }
    cn = cf[q.f1];
    publish();
  }
  for (; f >= q.f0; --f) step(f, false, 0.f);

#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = tid + k * nth;
    if (j < N) {
      const int i = q.node_off + j;
      beta[j + 1] = make_double2(bT[k], bB[k]);
      acc.occ[i] = occ[k]; acc.tsum[i] = ts[k]; acc.peak[i] = pk[k]; acc.peak_frame[i] = pf[k]; acc.visit[i] = vis[k];
    }
  }
}

constexpr int SUM_LDS_MAX = 160 * 1024 - 1024;   // what an instantiation may be launched with: a workgroup's LDS less the static part
static_assert((CTC_GRAPH_MAX_NODES + 1) * (int)sizeof(double2) <= SUM_LDS_MAX, "one row of {T, B} in fp64 fits the LDS");
static_assert(2 * CTC_GRAPH_MAX_NODES * (int)sizeof(double) <= SUM_LDS_MAX, "two rows of beta(T) in fp64 fit the LDS");
// the packing of `meta`: an arc index + 1 in 16 bits, a degree in 7
static_assert(CTC_GRAPH_MAX_ARCS + 1 <= 0xffff && CTC_GRAPH_MAX_IN_DEGREE <= 127, "meta packs the arc start into 16 bits, the degree into 7");

template <int NPT>
int launch_forward(hipStream_t s, int n_seq, int threads, size_t lds, const GraphSeq* seqs, const float* lp, int ld, int r0, const int* rows,
                   const int* node_tok, const int* arc_off, const unsigned* arcs, const unsigned* rem, int blank, double* alpha, double* csum,
                   float* coff, float* arows, int slots, int single) {
  // per launch, a host call of microseconds: the attribute belongs to the current device, and engines on several devices share this code
  RVB_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_graph_sum_forward_kernel<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, SUM_LDS_MAX));
  ctc_graph_sum_forward_kernel<NPT><<<n_seq, threads, lds, s>>>(seqs, lp, ld, r0, rows, node_tok, arc_off, arcs, rem, blank, alpha, csum, coff,
                                                               arows, slots, single);
  return OK;
}

template <int NPT>
int launch_backward(hipStream_t s, int n_seq, int threads, size_t lds, const GraphSeq* seqs, const float* lp, int ld, int r0, const int* rows,
                    const int* node_tok, const int* succ_off, const unsigned* succs, const uint8_t* fin, int blank, double* beta,
                    const float* coff, const float* arows, const float* llhat, GsAcc acc, int slots) {
  RVB_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_graph_sum_backward_kernel<NPT>, hipFuncAttributeMaxDynamicSharedMemorySize, SUM_LDS_MAX));
  ctc_graph_sum_backward_kernel<NPT><<<n_seq, threads, lds, s>>>(seqs, lp, ld, r0, rows, node_tok, succ_off, succs, fin, blank, beta, coff, arows,
                                                                llhat, acc, slots);
  return OK;
}

}  // namespace

int ctc_graph_sum_forward(hipStream_t s, const GraphSeq* seqs, int n_seq, int max_N, const float* lp, int ld, int r0, const int* rows,
                          const int* node_tok, const int* arc_off, const unsigned* arcs, const unsigned* rem, int blank, double* alpha,
                          double* csum, float* coff, float* arows) {
  if (n_seq <= 0) return OK;
  if (max_N < 1 || max_N > CTC_GRAPH_MAX_NODES) { set_error("ctc_graph_sum_forward: nodes out of range"); return E_ARG; }
  const int npt = ctc_graph_npt_for(max_N);
  const int threads = ctc_threads(max_N, npt);
  const int slots = max_N + 1;
  const int single = (size_t)2 * slots * sizeof(double2) > (size_t)SUM_LDS_MAX;      // above 5087 nodes: one buffer, two barriers per frame
  const size_t lds = (size_t)(single ? 1 : 2) * slots * sizeof(double2);
#define RVB_GSUM_(NPT) RVB_TRY(launch_forward<NPT>(s, n_seq, threads, lds, seqs, lp, ld, r0, rows, node_tok, arc_off, arcs, rem, blank, alpha, csum, coff, arows, slots, single))
  if (npt == 1) RVB_GSUM_(1);
  else if (npt == 2) RVB_GSUM_(2);
  else if (npt == 4) RVB_GSUM_(4);
  else RVB_GSUM_(8);
#undef RVB_GSUM_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int ctc_graph_sum_loglik(hipStream_t s, const GraphSeq* seqs, int n_seq, const int* finals, const double* alpha, const double* csum,
                         double* loglik, float* llhat) {
  if (n_seq <= 0) return OK;
  ctc_graph_sum_loglik_kernel<<<n_seq, 64, 0, s>>>(seqs, finals, alpha, csum, loglik, llhat);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int ctc_graph_sum_backward(hipStream_t s, const GraphSeq* seqs, int n_seq, int max_N, const float* lp, int ld, int r0, const int* rows,
                           const int* node_tok, const int* succ_off, const unsigned* succs, const uint8_t* fin, int blank, double* beta,
                           const float* coff, const float* arows, const float* llhat, float* occ, float* tsum, float* peak, int* peak_frame,
                           float* visit) {
  if (n_seq <= 0) return OK;
  if (max_N < 1 || max_N > CTC_GRAPH_MAX_NODES) { set_error("ctc_graph_sum_backward: nodes out of range"); return E_ARG; }
  const int npt = ctc_graph_npt_for(max_N);
  const int threads = ctc_threads(max_N, npt);
  const int slots = max_N;
  const size_t lds = (size_t)2 * slots * sizeof(double);
  const GsAcc acc{occ, tsum, peak, peak_frame, visit};
#define RVB_GSUM_(NPT) RVB_TRY(launch_backward<NPT>(s, n_seq, threads, lds, seqs, lp, ld, r0, rows, node_tok, succ_off, succs, fin, blank, beta, coff, arows, llhat, acc, slots))
  if (npt == 1) RVB_GSUM_(1);
  else if (npt == 2) RVB_GSUM_(2);
  else if (npt == 4) RVB_GSUM_(4);
  else RVB_GSUM_(8);
#undef RVB_GSUM_
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcGraphScorer::plan(const char* who, const int32_t* node_tokens, const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds,
                         const uint8_t* is_final, int n_seq, const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id,
                         bool posteriors) {
  RVB_TRY(lat.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, n_seq, seq_rows, V, blank_id));
  post = posteriors;
  const std::string w(who);
  h_rem.clear(); h_succ_off.clear(); h_succs.clear(); h_fin.clear();
  std::vector<uint32_t> remT, remB;
  std::vector<int32_t> fill;
  for (int i = 0; i < n_seq; ++i) {
    const GraphSeq& q = lat.seq[i];
    const int N = q.N;
    const std::string at = w + ": sequence " + std::to_string(i) + ": ";
    const int32_t* y = node_tokens + q.node_off;
    const int32_t* po = pred_off + q.node_off + i;
    const int32_t* pr = preds + q.arc_off;
    const uint8_t* fin = is_final + q.node_off;
    for (int j = 0; j < N; ++j)
      if (y[j] == RVB_CTC_WILDCARD) {
        set_error(at + "node " + std::to_string(j) + ": a wildcard has no full-sum score (the maximum over the vocabulary is no probability)");
        return E_ARG;
      }
    // the fewest frames from T_j / B_j to a final end; successors come later in the order, so one descending pass settles them
    remT.assign(N, REM_NEVER); remB.assign(N, REM_NEVER);
    std::vector<int32_t> out_deg(N + 1, 0);
    uint32_t rem_start = REM_NEVER;
    for (int j = N - 1; j >= 0; --j) {
      if (fin[j]) remT[j] = remB[j] = 0;
      for (int a = po[j]; a < po[j + 1]; ++a) {
        const int p = pr[a];
        if (remT[j] == REM_NEVER) { if (p >= 0) ++out_deg[p]; continue; }
        if (p < 0) { rem_start = std::min(rem_start, remT[j] + 1); continue; }
        ++out_deg[p];
        remT[p] = std::min(remT[p], remT[j] + (y[p] != y[j] ? 1u : 2u));
        remB[p] = std::min(remB[p], remT[j] + 1);
      }
    }
    if (posteriors)
      for (int j = 0; j < N; ++j)
        if (out_deg[j] > CTC_GRAPH_MAX_IN_DEGREE) {
          set_error(at + "node " + std::to_string(j) + ": out-degree " + std::to_string(out_deg[j]) + " exceeds the cap of " +
                    std::to_string(CTC_GRAPH_MAX_IN_DEGREE) + " successors per node (posteriors sweep the graph backwards)");
          return E_UNSUPPORTED;
        }
    if (rem_start == REM_NEVER || (int64_t)rem_start > (int64_t)q.T) {
      set_error(at + "infeasible: no path of " + std::to_string(q.T) + " frames through the graph ends in a final node with a finite score");
      return E_ARG;
    }
    for (int j = 0; j < N; ++j) h_rem.push_back(remT[j] | remB[j] << 16);
    h_rem.push_back(rem_start);
    h_fin.insert(h_fin.end(), fin, fin + N);
    // the transposed arcs: per node its successors, ascending; N + 1 offsets per lattice, the words from the lattice's arc_off
    const size_t o0 = h_succ_off.size();
    int32_t run = 0;
    for (int j = 0; j < N; ++j) { h_succ_off.push_back(run); run += out_deg[j]; }
    h_succ_off.push_back(run);
    h_succs.resize((size_t)q.arc_off + po[N], 0u);
    fill.assign(h_succ_off.begin() + o0, h_succ_off.begin() + o0 + N);
    for (int j = 0; j < N; ++j)
      for (int a = po[j]; a < po[j + 1]; ++a) {
        const int p = pr[a];
        if (p >= 0) h_succs[(size_t)q.arc_off + fill[p]++] = (uint32_t)j | (y[p] != y[j] ? ARC_T : 0u);
      }
  }
  return OK;
}

int CtcGraphScorer::begin(hipStream_t s) {
  const size_t n_seq = lat.seq.size(), n_nodes = lat.h_tokens.size();
  RVB_TRY(lat.d_tokens.ensure(n_nodes * 4));
  RVB_TRY(lat.d_arc_off.ensure(lat.h_arc_off.size() * 4));
  RVB_TRY(lat.d_arcs.ensure(lat.h_arcs.size() * 4));
  RVB_TRY(lat.d_finals.ensure(lat.h_finals.size() * 4));
  RVB_TRY(lat.d_rows.ensure(lat.h_rows.size() * 4));
  RVB_TRY(lat.d_seqs.ensure(n_seq * sizeof(GraphSeq)));
  RVB_TRY(lat.d_alpha.ensure(lat.alpha_floats * 8));          // the aligner's layout, a double where it keeps a float
  RVB_TRY(d_rem.ensure(h_rem.size() * 4));
  RVB_TRY(d_csum.ensure(n_seq * 8));
  RVB_TRY(d_loglik.ensure(n_seq * 8));
  RVB_TRY(d_llhat.ensure(n_seq * 4));
  if (post) {
    const size_t row_bytes = lat.bp_bytes * 4;     // the layout of the aligner's back-pointer bytes at 4 bytes per frame and node
    if (int r = d_arows.ensure(row_bytes)) {
      set_error("ctc score graph: " + std::to_string(row_bytes) + " bytes of alpha rows (4 bytes per frame and node) do not fit: " + last_error());
      return r;
    }
    RVB_TRY(d_coff.ensure((size_t)lat.total_frames * 4));
    RVB_TRY(d_beta.ensure(lat.alpha_floats * 8));
    RVB_TRY(d_acc.ensure(n_nodes * 20));
    RVB_TRY(d_succ_off.ensure(h_succ_off.size() * 4));
    RVB_TRY(d_succs.ensure(std::max<size_t>(h_succs.size(), 1) * 4));
    RVB_TRY(d_fin.ensure(h_fin.size()));
    RVB_HIP_CHECK(hipMemcpyAsync(d_succ_off.p, h_succ_off.data(), h_succ_off.size() * 4, hipMemcpyHostToDevice, s));
    if (!h_succs.empty()) RVB_HIP_CHECK(hipMemcpyAsync(d_succs.p, h_succs.data(), h_succs.size() * 4, hipMemcpyHostToDevice, s));
    RVB_HIP_CHECK(hipMemcpyAsync(d_fin.p, h_fin.data(), h_fin.size(), hipMemcpyHostToDevice, s));
  }
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_tokens.p, lat.h_tokens.data(), n_nodes * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_arc_off.p, lat.h_arc_off.data(), lat.h_arc_off.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_arcs.p, lat.h_arcs.data(), lat.h_arcs.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_finals.p, lat.h_finals.data(), lat.h_finals.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_rows.p, lat.h_rows.data(), lat.h_rows.size() * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_rem.p, h_rem.data(), h_rem.size() * 4, hipMemcpyHostToDevice, s));
  for (auto& q : lat.seq) q.f0 = q.f1 = 0;
  return OK;
}

int CtcGraphScorer::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  bool any;
  RVB_TRY(slab_window("ctc score graph", false, lat.seq, lat.h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, lat.d_seqs.p, lat.seq));
  return ctc_graph_sum_forward(s, lat.d_seqs.as<GraphSeq>(), (int)lat.seq.size(), lat.max_N, lp, ld, r0, lat.d_rows.as<int>(),
                               lat.d_tokens.as<int>(), lat.d_arc_off.as<int>(), lat.d_arcs.as<unsigned>(), d_rem.as<unsigned>(), lat.blank,
                               lat.d_alpha.as<double>(), d_csum.as<double>(), post ? d_coff.as<float>() : nullptr,
                               post ? d_arows.as<float>() : nullptr);
}

int CtcGraphScorer::finish_forward(hipStream_t s, double* loglik) {
  RVB_TRY(slab_covered("ctc score graph", false, lat.seq));
  for (auto& q : lat.seq) q.f0 = q.f1 = q.T;       // the backward sweep starts above the last frame
  RVB_TRY(ctc_graph_sum_loglik(s, lat.d_seqs.as<GraphSeq>(), (int)lat.seq.size(), lat.d_finals.as<int>(), lat.d_alpha.as<double>(),
                                d_csum.as<double>(), d_loglik.as<double>(), d_llhat.as<float>()));
  RVB_HIP_CHECK(hipMemcpyAsync(loglik, d_loglik.p, lat.seq.size() * 8, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  return slab_feasible("ctc score graph", lat.seq, loglik, "through the graph ends in a final node");
}

int CtcGraphScorer::advance_backward(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  if (!post) { set_error("ctc score graph: backward sweep without alpha rows"); return E_STATE; }
  bool any;
  RVB_TRY(slab_window("ctc score graph", true, lat.seq, lat.h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, lat.d_seqs.p, lat.seq));
  float* acc = d_acc.as<float>();
  const size_t n = lat.h_tokens.size();
  return ctc_graph_sum_backward(s, lat.d_seqs.as<GraphSeq>(), (int)lat.seq.size(), lat.max_N, lp, ld, r0, lat.d_rows.as<int>(),
                                lat.d_tokens.as<int>(), d_succ_off.as<int>(), d_succs.as<unsigned>(), d_fin.as<uint8_t>(), lat.blank,
                                d_beta.as<double>(), d_coff.as<float>(), d_arows.as<float>(), d_llhat.as<float>(), acc, acc + n, acc + 2 * n,
                                (int*)(acc + 3 * n), acc + 4 * n);
}

int CtcGraphScorer::finish_backward(hipStream_t s, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  RVB_TRY(slab_covered("ctc score graph", true, lat.seq));
  const size_t n = lat.h_tokens.size();
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

void CtcGraphScorer::release() {
  lat.release();
  for (DevBuf* b : {&d_rem, &d_csum, &d_loglik, &d_llhat, &d_coff, &d_arows, &d_beta, &d_acc, &d_succ_off, &d_succs, &d_fin}) b->release();
}

}  // namespace rvb
