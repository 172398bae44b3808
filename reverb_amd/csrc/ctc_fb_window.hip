// Windowed CTC forward-backward: the full-sum score (and per-token posteriors) of a transcript of any length over a lattice that
// arrives in several encoded batches.  The recurrences, the normalisation (the offset c[t] = the row maximum over the states that can
// still reach the end, C summed in fp64, ll^, the division by Z[t + 1]) and the per-token accumulators are those of
// ctc_forward_backward.hip; the window mechanics (one workgroup, SPT = 4 / 16 / 32 by ctc_spt_for(W), thread tid owns the states
// lo + tid * SPT ..., lo a field of the launch's descriptor, one __syncthreads() per frame) are those of ctc_viterbi_window.hip.
//
// Band semantics (shared with tests/ctc_score_window_ref.py).  lo_of[t] is the window of the launch that computes frame t: a multiple
// of 32 that never decreases.
//   * cell (t, s) is alive iff lo_of[t] <= s < min(lo_of[t] + W, S);
//   * a transition (t-1, s') -> (t, s) counts iff both cells are alive AND s' >= lo_of[t]: the forward launch reads predecessors only
//     from its own window, below it is -inf;
//   * the full sum runs over the paths made of counted transitions.
//
//   alpha, beta  fp32 [S_pad], the WHOLE lattice, -inf at begin(); a launch reads its window's states and writes them back.
//   arows, c     with posteriors the forward launch stores c[t] and its normalised row WINDOW-RELATIVE: T x W x 4 bytes.
//   best         after its last frame the forward launch reduces its normalised row, over the window states that can still reach the
//                end (the set the row's normaliser runs over), to the FIRST maximum (lowest state on a tie; -1 if none is finite):
//                8 bytes the host reads back to place the next window (ctc_window_next_lo).
//   backward     replays the recorded launches in reverse, each with its own lo.  The descriptor also carries lo_next, the lo of the
//                launch that owns frame f1: at the launch's first step (frame f1 - 1) every state s < lo_next gets -inf, the mirror
//                image of the forward cut (without it the posteriors of a frame no longer sum to 1 at a window move), and the two
//                states above the window's last, alive at frame f1 when the window has moved, are read from beta in HBM for that one
//                step; after it the right neighbour of the window's last state is -inf.
//
// With W >= S_pad the window never moves, every launch is the plain kernel's and the results are rvb_ctc_score's bit for bit, however
// the launches are cut: alpha, beta, C and Z are carried exactly.  Every loop is bounded by T, SPT, W or the waves of a workgroup.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace rvb {

namespace {

// log(exp(x0) + exp(x1) + exp(x2)); -inf when all three are
__device__ __forceinline__ float lse3(float x0, float x1, float x2) {
  const float m = fmaxf(fmaxf(x0, x1), x2);
  const float mm = m > -INFINITY ? m : 0.f;
  return mm + logf(expf(x0 - mm) + expf(x1 - mm) + expf(x2 - mm));
}
__device__ __forceinline__ float lse2(float x0, float x1) {
  const float m = fmaxf(x0, x1);
  const float mm = m > -INFINITY ? m : 0.f;
  return mm + logf(expf(x0 - mm) + expf(x1 - mm));
}

struct FbwSeg {            // one launch: the lattice, its window and the frames to advance over
  int L, S, T, W;          // tokens, states 2 L + 1, frames of the whole lattice, states of the window (a multiple of 32)
  int lo;                  // first state of the window (a multiple of 32; 0 in the launch that holds frame 0)
  int lo_next;             // backward only: the window of the launch that owns frame f1 (lo when f1 == T)
  int f0, f1;              // lattice frames of this launch (forward: f0 == 0 initialises; backward: f1 == T starts the sweep)
  int fbase;               // the lattice frame of rows[0]: frame f reads row rows[f - fbase] - r0 of lp
};
struct FbwBest { int state; float value; };

template <int SPT>
__global__ __launch_bounds__(1024) void ctc_fb_window_forward_kernel(const FbwSeg q, const float* __restrict__ lp, int ld, int r0,
                                                                     const int* __restrict__ rows, const int* __restrict__ y, int blank,
                                                                     float* __restrict__ alpha, double* __restrict__ csum,
                                                                     float* __restrict__ coff, float* __restrict__ arows,
                                                                     FbwBest* __restrict__ best_out) {
  constexpr int NT = SPT / 2;                      // tokens per thread: local state 2k + 1 is token s0 / 2 + k, even states are blank
  __shared__ float bnd[2][1024];                   // per thread: alpha of its last state
  __shared__ float wmax[2][16];                    // per wave: maximum of the row
  __shared__ float red_v[16];
  __shared__ int red_s[16];
  if (q.f0 >= q.f1) return;                        // uniform over the workgroup
  const int tid = threadIdx.x, nw = blockDim.x >> 6;
  const int s0 = q.lo + tid * SPT;                 // first state of this thread in the lattice
  const float NEG = -INFINITY;
  const bool mine = tid * SPT < q.W;               // the launch rounds the threads up to whole waves: some own nothing
  const int nvalid = mine ? min(max(q.S - s0, 0), SPT) : 0;     // states of this thread that exist
  const long long stride = q.W;                    // floats per stored row: window-relative
  const bool keep = arows != nullptr && mine;
  float* arow = keep ? arows + tid * SPT : nullptr;

  unsigned tok[NT];                                // byte offset of each token's column in a row of lp
  unsigned skip = 0;                               // bit k: state 2k + 1 may be entered from two states below
  {
    int prev = (s0 >= 2 && s0 / 2 - 1 < q.L) ? y[s0 / 2 - 1] : -1;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int i = s0 / 2 + k;
      const bool have = i < q.L;
      const int id = have ? y[i] : blank;          // a column that exists, for the states past S - 1
      if (have && i >= 1 && id != prev) skip |= 1u << k;
      prev = id;
      tok[k] = (unsigned)id * 4u;
    }
  }

  float a[SPT];
  float eb, et[NT];                                // emissions of the frame about to be computed; refilled right after their use
  auto row_of = [&](int fr) { return rows[min(fr, q.f1 - 1) - q.fbase] - r0; };   // past the last frame of this launch: clamped
  auto fill = [&](int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
#pragma unroll
    for (int k = 0; k < NT; ++k) et[k] = *(const float*)(row + tok[k]);
  };
  auto store_row = [&](int fr) {
    if (!keep) return;
    float4* dst = (float4*)(arow + (size_t)fr * stride);
#pragma unroll
    for (int j = 0; j < SPT; j += 4) dst[j / 4] = make_float4(a[j], a[j + 1], a[j + 2], a[j + 3]);
  };
  int par = 0;
  auto publish = [&](int fr) {                     // boundary value and row maximum of frame fr, just computed, then its barrier
    const int live = q.S - 2 * (q.T - fr) - s0;    // the maximum runs over the states that can still reach the end
    float m = NEG;
#pragma unroll
    for (int j = 0; j < SPT; ++j) m = fmaxf(m, j >= live ? a[j] : NEG);
    m = wave_max(m);
    if ((tid & 63) == 0) wmax[par][tid >> 6] = m;
    bnd[par][tid] = a[SPT - 1];
    __syncthreads();
  };

  int f = q.f0;
  double C = 0.0;
  fill(row_of(f));
  if (f == 0) {                                    // the window of frame 0 starts at state 0
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = NEG;
    if (tid == 0) { a[0] = eb; a[1] = et[0]; if (coff) coff[0] = 0.f; }
    store_row(0);
    f = 1;
    fill(row_of(1));
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = j < nvalid ? alpha[s0 + j] : NEG;
    if (tid == 0) C = csum[0];
  }
  publish(f - 1);

  for (; f < q.f1; ++f) {
    const char* row = (const char*)(lp + (size_t)row_of(f + 1) * ld);
    const float left = tid > 0 ? bnd[par][tid - 1] : NEG;       // below the window: -inf
    float m = wmax[par][0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, wmax[par][w]);
    const float c = m > NEG ? m : 0.f;             // the offset of this frame: the maximum of the row before it
#pragma unroll
    for (int j = SPT - 1; j >= 0; --j) {           // downwards: a[j-1], a[j-2] still hold frame f - 1
      const float x1 = j >= 1 ? a[j - 1] : left;
      float v;
      if (j & 1) {
        const float x2 = ((skip >> (j >> 1)) & 1u) ? (j >= 2 ? a[j - 2] : left) : NEG;
        v = (lse3(a[j], x1, x2) + et[j >> 1]) - c;
        et[j >> 1] = *(const float*)(row + tok[j >> 1]);
      } else {
        v = (lse2(a[j], x1) + eb) - c;
      }
      a[j] = j < nvalid ? v : NEG;                 // states past S - 1 stay out of the maximum and of the stored row
    }
    eb = *(const float*)(row + (unsigned)blank * 4u);
    if (tid == 0) { C += (double)c; if (coff) coff[f] = c; }
    store_row(f);
    par ^= 1;
    publish(f);
  }
  if (tid == 0) csum[0] = C;

  // the first maximum of the last row over the states its normaliser runs over: lowest state on a tie, -1 when none is finite
  const int live = q.S - 2 * (q.T - (q.f1 - 1)) - s0;
  float bv = NEG;
  int bs = -1;
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < nvalid) {
      alpha[s0 + j] = a[j];
      if (j >= live && a[j] > bv) { bv = a[j]; bs = s0 + j; }
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
    for (int w = 1; w < nw; ++w)
      if (red_v[w] > bv || (red_v[w] == bv && (unsigned)red_s[w] < (unsigned)bs)) { bv = red_v[w]; bs = red_s[w]; }
    best_out->state = bs;
    best_out->value = bv;
  }
}

// per-token reductions of the posteriors, carried in HBM between launches (initialised by the host: 0, 0, -1, 0)
struct FbwAcc { float* occ; float* tsum; float* peak; int* peak_frame; };

template <int SPT>
__global__ __launch_bounds__(1024) void ctc_fb_window_backward_kernel(const FbwSeg q, const float* __restrict__ lp, int ld, int r0,
                                                                      const int* __restrict__ rows, const int* __restrict__ y, int blank,
                                                                      float* __restrict__ beta, const float* __restrict__ cf,
                                                                      const float* __restrict__ arows, const float* __restrict__ llhat,
                                                                      float* __restrict__ zcarry, FbwAcc acc) {
  constexpr int NT = SPT / 2;
  constexpr int CH = SPT < 32 ? SPT : 8;           // states whose alpha is loaded together (32 per thread: in pieces, for the registers)
  __shared__ float2 bnd[2][1024];                  // per thread: beta of its first two states (what the left neighbour's last two read)
  __shared__ float wsum[2][16];                    // per wave: sum of exp(gamma) of the row before normalisation
  if (q.f0 >= q.f1) return;
  const int tid = threadIdx.x, nw = blockDim.x >> 6;
  const int s0 = q.lo + tid * SPT;
  const float NEG = -INFINITY;
  // the bounds in the plain kernel's own form (the window's end for the lattice's, the window-relative row): written as a predicate
  // on the thread they make the compiler fuse other multiply-adds of the per-token sums than it fuses there, and the bits differ
  const int s_end = min(q.S, q.lo + q.W);          // one past the last state of this launch that exists
  const int nvalid = min(max(s_end - s0, 0), SPT);
  const long long stride = q.W;
  const bool have_row = tid * SPT + SPT <= stride; // else: this thread owns nothing of the window (the launch rounds up to whole waves)
  const float* arow = arows + (have_row ? tid * SPT : 0);
  const bool first = q.f1 == q.T;                  // this launch starts the sweep at the last frame
  const bool moved = !first && q.lo_next > q.lo;   // frame f1 belongs to a window further up

  unsigned tok[NT];
  unsigned fskip = 0;                              // bit k: state 2k + 1 may be left to two states above
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int i = s0 / 2 + k;
    const bool have = i < q.L;
    const int id = have ? y[i] : blank;
    if (i + 1 < q.L && y[i + 1] != id) fskip |= 1u << k;
    tok[k] = (unsigned)id * 4u;
  }

  float b[SPT];
  float eb, et[NT];
  float occ[NT], ts[NT], pk[NT];
  int pf[NT];
  auto row_of = [&](int fr) { return rows[max(fr, q.f0) - q.fbase] - r0; };      // below the first frame of this launch: clamped
  auto fill = [&](int r) {
    const char* row = (const char*)(lp + (size_t)r * ld);
    eb = *(const float*)(row + (unsigned)blank * 4u);
#pragma unroll
    for (int k = 0; k < NT; ++k) et[k] = *(const float*)(row + tok[k]);
  };
  int par = 0;
  auto publish = [&](float z) {
    z = wave_sum(z);
    if ((tid & 63) == 0) wsum[par][tid >> 6] = z;
    bnd[par][tid] = make_float2(b[0], b[1]);
    __syncthreads();
  };
  // one frame.  init: frame T - 1, whose b^ is lp - ll^ in the two end states; else the recursion from the b^ of frame f + 1
  float cn = 0.f;                                  // c[f + 1] of the frame about to be computed, read one frame ahead
  float2 top = make_float2(NEG, NEG);              // above the last thread's states: -inf, but for the first step after a move (below)
  auto step = [&](int f, bool init, float ll) {
    const char* row = (const char*)(lp + (size_t)row_of(f - 1) * ld);
    const float c = cn;
    cn = cf[f];
    float2 right = top;
    top = make_float2(NEG, NEG);
    float inv = 1.f;
    if (!init) {
      if (tid + 1 < (int)blockDim.x) right = bnd[par][tid + 1];
      float z = wsum[par][0];
      for (int w = 1; w < nw; ++w) z += wsum[par][w];
      inv = z > 0.f ? 1.f / z : 0.f;               // Z[f + 1]: what the common rounding of both sweeps has made of 1
    }
    const float* ar = arow + (size_t)f * stride;
    const float tf = (float)f;
    float zloc = 0.f;
#pragma unroll
    for (int j0 = 0; j0 < SPT; j0 += CH) {
      float av[CH];
#pragma unroll
      for (int j = 0; j < CH; j += 4) {
        const float4 v = have_row ? *(const float4*)(ar + j0 + j) : make_float4(NEG, NEG, NEG, NEG);
        av[j] = v.x; av[j + 1] = v.y; av[j + 2] = v.z; av[j + 3] = v.w;
      }
#pragma unroll
      for (int jj = 0; jj < CH; ++jj) {            // upwards: b[j+1], b[j+2] still hold frame f + 1
        const int j = j0 + jj;
        float u;
        if (init) {
          u = (s0 + j == q.S - 1 || s0 + j == q.S - 2) ? -ll : NEG;
        } else {
          const float y1 = j + 1 < SPT ? b[j + 1 < SPT ? j + 1 : 0] : right.x;
          if (j & 1) {
            const float y2 = ((fskip >> (j >> 1)) & 1u) ? (j + 2 < SPT ? b[j + 2 < SPT ? j + 2 : 0] : right.y) : NEG;
            u = lse3(b[j], y1, y2) - c;
          } else {
            u = lse2(b[j], y1) - c;
          }
        }
        if (j >= nvalid) u = NEG;
        const float p = expf(av[jj] + u);          // exp(gamma) before normalisation; 0 where alpha or beta is -inf
        zloc += p;
        if (j & 1) {
          const int k = j >> 1;
          const float g = p * inv;
          occ[k] += g;
          ts[k] += g * tf;
          if (g >= pk[k]) { pk[k] = g; pf[k] = f; }   // frames descend: >= keeps the first frame of a tie
          b[j] = u + et[k];
          et[k] = *(const float*)(row + tok[k]);
        } else {
          b[j] = u + eb;
        }
      }
    }
    eb = *(const float*)(row + (unsigned)blank * 4u);
    par ^= 1;
    publish(zloc);
  };

  int f = q.f1 - 1;
  fill(row_of(f));
  if (first) {                                     // the accumulators start as the host has set them in HBM: 0, 0, -1, 0
#pragma unroll
    for (int k = 0; k < NT; ++k) { occ[k] = 0.f; ts[k] = 0.f; pk[k] = -1.f; pf[k] = 0; }
#pragma unroll
    for (int j = 0; j < SPT; ++j) b[j] = NEG;
    step(f, true, llhat[0]);
    --f;
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j) b[j] = j < nvalid ? beta[s0 + j] : NEG;
#pragma unroll
    for (int k = 0; k < NT; ++k) {                 // the window's tokens; the others are untouched
      const int i = s0 / 2 + k;
      const bool have = have_row && i < q.L;
      occ[k] = have ? acc.occ[i] : 0.f;
      ts[k] = have ? acc.tsum[i] : 0.f;
      pk[k] = have ? acc.peak[i] : -1.f;
      pf[k] = have ? acc.peak_frame[i] : 0;
    }
    cn = cf[q.f1];
    // the Z the previous launch ended with, republished as wave 0's sum: adding the zeros of the other waves leaves its bits alone
    if ((tid & 63) == 0) wsum[0][tid >> 6] = tid == 0 ? zcarry[0] : 0.f;
    // The first step after a move.  lo_next is a thread boundary (a multiple of 32): the transitions from a state below lo_next to one
    // at or above it are what the thread below the boundary reads from its right neighbour, so that neighbour publishes -inf (the
    // cut; the states below hold -inf of their own, nothing of frame f1 was alive there).  The two states above the window's last are
    // alive at frame f1 (< lo_next + W <= S_pad): the first thread that owns nothing publishes them from HBM (a window of 1024
    // threads: its last thread reads them itself).  After this step every publish is the plain one.
    float2 pub = make_float2(b[0], b[1]);
    if (moved && s0 == q.lo_next) pub = make_float2(NEG, NEG);
    if (moved && tid * SPT == q.W) pub = make_float2(beta[q.lo + q.W], beta[q.lo + q.W + 1]);
    if (moved && tid + 1 == (int)blockDim.x && (tid + 1) * SPT == q.W) top = make_float2(beta[q.lo + q.W], beta[q.lo + q.W + 1]);
    bnd[0][tid] = pub;
    __syncthreads();
  }
  for (; f >= q.f0; --f) step(f, false, 0.f);

#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < nvalid) beta[s0 + j] = b[j];
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int i = s0 / 2 + k;
    if (have_row && i < q.L) {
      acc.occ[i] = occ[k]; acc.tsum[i] = ts[k];
      acc.peak[i] = pk[k]; acc.peak_frame[i] = pf[k];
    }
  }
  if (tid == 0) {
    float z = wsum[par][0];
    for (int w = 1; w < nw; ++w) z += wsum[par][w];
    zcarry[0] = z;
  }
}

int fbw_forward(hipStream_t s, const FbwSeg& q, const float* lp, int ld, int r0, const int* rows, const int* tokens, int blank,
                float* alpha, double* csum, float* coff, float* arows, FbwBest* best) {
  const int spt = ctc_spt_for(q.W), threads = ctc_threads(q.W, spt);
  if (spt == 4) ctc_fb_window_forward_kernel<4><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, alpha, csum, coff, arows, best);
  else if (spt == 16) ctc_fb_window_forward_kernel<16><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, alpha, csum, coff, arows, best);
  else ctc_fb_window_forward_kernel<32><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, alpha, csum, coff, arows, best);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int fbw_backward(hipStream_t s, const FbwSeg& q, const float* lp, int ld, int r0, const int* rows, const int* tokens, int blank,
                 float* beta, const float* coff, const float* arows, const float* llhat, float* zcarry, const FbwAcc& acc) {
  const int spt = ctc_spt_for(q.W), threads = ctc_threads(q.W, spt);
  if (spt == 4) ctc_fb_window_backward_kernel<4><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, beta, coff, arows, llhat, zcarry, acc);
  else if (spt == 16) ctc_fb_window_backward_kernel<16><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, beta, coff, arows, llhat, zcarry, acc);
  else ctc_fb_window_backward_kernel<32><<<1, threads, 0, s>>>(q, lp, ld, r0, rows, tokens, blank, beta, coff, arows, llhat, zcarry, acc);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int fill32(hipStream_t s, void* p, float v, size_t n) {
  int bits;
  memcpy(&bits, &v, 4);
  RVB_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)p, bits, n, s));
  return OK;
}

const char* const WHO = "ctc score long";

}  // namespace

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcWindowScorer::plan(const char* who, const int32_t* tokens, int n_tokens, int64_t total_frames, int window_states, int V,
                          int blank_id) {
  CtcWindowAligner p;                              // its checks and words; no wildcards: RVB_CTC_WILDCARD is an id outside the vocabulary
  open = false;
  RVB_TRY(p.plan(who, tokens, n_tokens, total_frames, window_states, V, blank_id, false, 0.f));
  L = p.L; S = p.S; S_pad = p.S_pad; T = p.T; W = p.W; blank = p.blank;
  row_bytes = (size_t)T * (size_t)W * 4;
  h_tokens.swap(p.h_tokens);
  h_rows.clear();
  launches.clear();
  batches.clear();
  fed = fbase = 0; lo = 0; best = -1; back = 0; back_batch = 0; cursor = 0;
  forward_done = false; post = false;
  lo_force = nullptr; n_force = 0;
  return OK;
}

int CtcWindowScorer::launch_count(int slab_rows) const {
  const int seg = W / 4 > 32 ? W / 4 - 16 : std::max(W / 4, 1);
  int64_t n = 0;
  for (int64_t s0 = 0; s0 < T; s0 += slab_rows) n += (std::min<int64_t>(slab_rows, T - s0) + seg - 1) / seg;
  return (int)n;
}

int CtcWindowScorer::rows_fit() const {
  // lab hook (librvb_test.so only): pretend that more than RVB_CTC_SCORE_FAKE_NOMEM_ABOVE bytes of alpha rows do not fit
  if (const char* f = lab_env("RVB_CTC_SCORE_FAKE_NOMEM_ABOVE")) {
    if ((double)row_bytes > atof(f)) {
      set_error(std::string(WHO) + ": " + std::to_string(row_bytes) + " bytes of alpha rows (4 bytes per frame and window state) do not fit: " +
                "hipMalloc refused (RVB_CTC_SCORE_FAKE_NOMEM_ABOVE)");
      return E_NOMEM;
    }
  }
  return OK;
}

int CtcWindowScorer::begin(hipStream_t s, bool posteriors) {
  post = posteriors;
  if (post) RVB_TRY(rows_fit());
  RVB_TRY(d_tokens.ensure((size_t)L * 4));
  RVB_TRY(d_alpha.ensure((size_t)S_pad * 4));
  RVB_TRY(d_seq.ensure(sizeof(VitSeq)));
  RVB_TRY(d_csum.ensure(8));
  RVB_TRY(d_loglik.ensure(8));
  RVB_TRY(d_llhat.ensure(4));
  RVB_TRY(d_best.ensure(sizeof(FbwBest)));
  if (post) {
    if (int r = d_arows.ensure(row_bytes)) {
      set_error(std::string(WHO) + ": " + std::to_string(row_bytes) + " bytes of alpha rows (4 bytes per frame and window state) do not fit: " +
                last_error());
      return r;
    }
    RVB_TRY(d_coff.ensure((size_t)T * 4));
    RVB_TRY(d_beta.ensure((size_t)S_pad * 4));
    RVB_TRY(d_z.ensure(4));
    RVB_TRY(d_acc.ensure((size_t)L * 16));
  }
  VitSeq q{};                                      // what ctc_fb_loglik reads: the end states of the one lattice
  q.L = L; q.S = S; q.T = T;
  RVB_HIP_CHECK(hipMemcpyAsync(d_tokens.p, h_tokens.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(d_seq.p, &q, sizeof(q), hipMemcpyHostToDevice, s));
  RVB_TRY(fill32(s, d_alpha.p, -INFINITY, (size_t)S_pad));
  RVB_HIP_CHECK(hipMemsetAsync(d_csum.p, 0, 8, s));
  if (post) {
    float* acc = d_acc.as<float>();
    RVB_TRY(fill32(s, d_beta.p, -INFINITY, (size_t)S_pad));
    RVB_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)L * 16, s));       // occupancy, frame-weighted sum, peak frame: 0
    RVB_TRY(fill32(s, acc + 2 * (size_t)L, -1.f, (size_t)L));       // peak posterior: below every posterior
  }
  RVB_HIP_CHECK(hipStreamSynchronize(s));          // q and h_tokens may go
  open = true;
  return OK;
}

int CtcWindowScorer::batch(hipStream_t s, const std::vector<int32_t>& rows) {
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

bool CtcWindowScorer::touches(int r0, int nrows) const {
  const auto a = std::lower_bound(h_rows.begin(), h_rows.end(), r0), b = std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows);
  return a != b;
}

int CtcWindowScorer::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  if (!open) { set_error(std::string(WHO) + ": feed before begin"); return E_STATE; }
  if (forward_done) { set_error(std::string(WHO) + ": feed after the forward sweep was finished"); return E_STATE; }
  const int b0 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0) - h_rows.begin());
  const int b1 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows) - h_rows.begin());
  if (b0 == b1) return OK;
  if (fbase + b0 != fed) { set_error(std::string(WHO) + ": slabs must arrive in row order"); return E_STATE; }
  // the launches are cut as CtcWindowAligner::advance cuts them: a path at the window's centre cannot leave through the top within one
  const int seg = W / 4 > 32 ? W / 4 - 16 : std::max(W / 4, 1);
  for (int g0 = fbase + b0, end = fbase + b1; g0 < end; g0 += seg) {
    const int g1 = std::min(g0 + seg, end);
    lo = ctc_window_next_lo(S, T, W, g0, g1, lo, best);
    if (lo_force && (int)launches.size() < n_force) lo = lo_force[launches.size()];   // lab: the schedule of the test
    FbwSeg q{L, S, T, W, lo, lo, g0, g1, fbase};
    RVB_TRY(fbw_forward(s, q, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), blank, d_alpha.as<float>(), d_csum.as<double>(),
                        post ? d_coff.as<float>() : nullptr, post ? d_arows.as<float>() : nullptr, d_best.as<FbwBest>()));
    FbwBest hb;
    RVB_HIP_CHECK(hipMemcpyAsync(&hb, d_best.p, sizeof(hb), hipMemcpyDeviceToHost, s));
    RVB_HIP_CHECK(hipStreamSynchronize(s));        // the one synchronisation of a launch: the next window depends on it
    best = hb.state;
    launches.push_back({g0, g1, lo, best});
    fed = g1;
  }
  return OK;
}

int CtcWindowScorer::finish_forward(hipStream_t s, double* loglik) {
  if (!open) { set_error(std::string(WHO) + ": loglik before begin"); return E_STATE; }
  if (fed != T) {
    set_error(std::string(WHO) + ": loglik before all " + std::to_string(T) + " frames were fed (" + std::to_string(fed) + " so far)");
    return E_STATE;
  }
  double ll = 0.0;
  RVB_TRY(ctc_fb_loglik(s, d_seq.as<VitSeq>(), 1, d_alpha.as<float>(), d_csum.as<double>(), d_loglik.as<double>(), d_llhat.as<float>()));
  RVB_HIP_CHECK(hipMemcpyAsync(&ll, d_loglik.p, 8, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  if (!(ll > -INFINITY)) {
    set_error(std::string(WHO) + ": infeasible: no path inside the window of " + std::to_string(W) + " states emits the transcript over " +
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
  if (loglik) *loglik = ll;
  return OK;
}

int CtcWindowScorer::batch_backward(hipStream_t s, const std::vector<int32_t>& rows) {
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

int CtcWindowScorer::advance_backward(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  if (!open) { set_error(std::string(WHO) + ": feed before begin"); return E_STATE; }
  if (!post) { set_error(std::string(WHO) + ": backward sweep without alpha rows"); return E_STATE; }
  if (!forward_done) { set_error(std::string(WHO) + ": the backward sweep starts after the forward sweep was finished"); return E_STATE; }
  const int b0 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0) - h_rows.begin());
  const int b1 = (int)(std::lower_bound(h_rows.begin(), h_rows.end(), r0 + nrows) - h_rows.begin());
  if (b0 == b1) return OK;
  if (fbase + b1 != back) { set_error(std::string(WHO) + ": the backward sweep takes the slabs in descending row order"); return E_STATE; }
  float* acc = d_acc.as<float>();
  const FbwAcc a{acc, acc + L, acc + 2 * (size_t)L, (int*)(acc + 3 * (size_t)L)};
  // the recorded launches that hold the slab's frames, last first, each with its own window; one that the slab holds only in part is
  // run in part, which changes nothing: beta, Z and the accumulators are carried exactly
  for (const int low = fbase + b0; back > low;) {
    while (cursor > 0 && launches[cursor - 1].f0 >= back) --cursor;
    const Launch& m = launches[cursor - 1];
    const int g1 = back, g0 = std::max(m.f0, low);
    const int lo_next = g1 == m.f1 && cursor < (int)launches.size() ? launches[cursor].lo : m.lo;
    FbwSeg q{L, S, T, W, m.lo, lo_next, g0, g1, fbase};
    RVB_TRY(fbw_backward(s, q, lp, ld, r0, d_rows.as<int>(), d_tokens.as<int>(), blank, d_beta.as<float>(), d_coff.as<float>(),
                         d_arows.as<float>(), d_llhat.as<float>(), d_z.as<float>(), a));
    back = g0;
  }
  return OK;
}

int CtcWindowScorer::finish_backward(hipStream_t s, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  if (!open) { set_error(std::string(WHO) + ": finish before begin"); return E_STATE; }
  if (!post) { set_error(std::string(WHO) + ": backward sweep without alpha rows"); return E_STATE; }
  if (!forward_done || back != 0) {
    set_error(std::string(WHO) + ": the backward sweep did not reach the first frame (" + std::to_string(forward_done ? back : T) +
              " frames to go)");
    return E_STATE;
  }
  const size_t n_tok = (size_t)L;
  std::vector<float> h(4 * n_tok);
  RVB_HIP_CHECK(hipMemcpyAsync(h.data(), d_acc.p, n_tok * 16, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  for (size_t k = 0; k < n_tok; ++k) {
    if (occupancy) occupancy[k] = h[k];
    if (mean_frame) mean_frame[k] = h[k] > 0.f ? h[n_tok + k] / h[k] : -1.f;    // no mass at all (only with -inf emissions): no frame
    if (peak_post) peak_post[k] = h[2 * n_tok + k];
  }
  if (peak_frame) memcpy(peak_frame, h.data() + 3 * n_tok, n_tok * 4);
  return OK;
}

void CtcWindowScorer::lo_per_frame(int32_t* lo_out) const {
  for (const Launch& m : launches)
    for (int t = m.f0; t < m.f1; ++t) lo_out[t] = m.lo;
}

void CtcWindowScorer::release() {
  for (DevBuf* b : {&d_tokens, &d_rows, &d_alpha, &d_seq, &d_csum, &d_loglik, &d_llhat, &d_best, &d_coff, &d_arows, &d_beta, &d_z, &d_acc})
    b->release();
  open = false;
}

}  // namespace rvb
