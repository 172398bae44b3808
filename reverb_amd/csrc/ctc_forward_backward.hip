// CTC full-sum scoring of a known transcript (the reference's CTC.forward, asr/wenet/transformer/ctc.py:65-104 = torch.nn.CTCLoss over
// the log-softmax of the CTC head, reported by bin/get_loss.py): the sibling of ctc_viterbi.hip with log-sum-exp in place of max, plus
// a backward sweep for per-token posteriors.  Extended sequence z = [b, y0, b, ..., y(L-1), b], S = 2L + 1 states.
//
//   alpha[0][0] = lp[0][b], alpha[0][1] = lp[0][y0], -inf elsewhere
//   alpha[t][s] = logsumexp(alpha[t-1][s], alpha[t-1][s-1] (, alpha[t-1][s-2] if z[s] != b and z[s] != z[s-2])) + lp[t][z[s]]
//   loglik      = logsumexp(alpha[T-1][S-1], alpha[T-1][S-2])
//   beta[T-1][s] = lp[T-1][z[s]] for s = S-1, S-2;  beta[t][s] = logsumexp(beta[t+1][s], beta[t+1][s+1] (, beta[t+1][s+2])) + lp[t][z[s]]
//   gamma[t][s] = alpha[t][s] + beta[t][s] - lp[t][z[s]] - loglik           (beta includes the emission of its own frame)
//
// Normalisation.  What the kernels carry is a^[t][s] = alpha[t][s] - C[t], C[t] = c[1] + ... + c[t], where c[t] is the workgroup
// maximum of the row a^[t-1] (0 for t = 0) over the states that can still reach the end, s >= S - 2 (T - (t-1)): the states that
// carry the likelihood then stay within a frame's gain of 0, whatever T is (a maximum over ALL states follows the paths that lag
// behind and can no longer finish, and leaves the live ones thousands of nats below it).  The maximum of a row is
// reduced inside each wave (no barrier), published beside the boundary values before the one barrier of its frame and combined by
// every thread after it, so the reduction adds no barrier.  c[t] is an fp32 value that is subtracted as it is; thread 0 sums the
// c[t] in fp64, so C[T-1] is exact to fp64 rounding and loglik = C[T-1] + logsumexp(a^[T-1][S-1], a^[T-1][S-2]).
// The backward sweep carries b^[t][s] = beta[t][s] - (loglik - C[t]), which makes gamma[t][s] = a^[t][s] + b^[t][s] - lp[t][z[s]]
// with no scalar left over: its recursion is b^[t][s] = logsumexp(b^[t+1][..]) - c[t+1] + lp[t][z[s]], from the c[t] the forward
// pass stored, and it starts from lp[T-1][z[s]] - ll^ with ll^ = loglik - C[T-1].  The rounding errors of both sweeps that are
// common to a whole row show up as Z[t] = sum_s exp(gamma[t][s]) != 1; Z changes by one frame's rounding from frame to frame, so the
// posteriors of frame t are divided by Z[t+1], which the previous step has reduced (again without a barrier of its own).
//
// Shape: as the Viterbi kernel.  ONE workgroup per lattice, SPT = 4 / 16 / 32 consecutive states per thread in registers, the
// neighbour's boundary values through double-buffered LDS, one __syncthreads() per frame, emissions of the next frame gathered
// before the barrier of this one.  Alpha (beta) lives in HBM between launches, so both sweeps advance slab by slab.  With
// posteriors the forward pass stores its normalised rows ([T][S_pad] fp32); the backward kernel reads the row of its frame and
// reduces occupancy, the frame-weighted sum, the peak posterior and its frame in registers of the thread that owns the token: no
// atomics.  exp / log are the accurate library functions.  A cell whose predecessors are all -inf stays -inf (the maximum is
// replaced by 0 before it is subtracted), so no NaN can arise.  Every loop is bounded by T, SPT or the waves of a workgroup.
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

// the alpha rows of a lattice share the layout of the Viterbi back-pointers (CtcAligner::plan): 4 bytes where those take 2 bits
__device__ __forceinline__ long long row_stride(const VitSeq& q) { return q.bp_stride * 4; }      // floats per frame = S padded to 32
__device__ __forceinline__ long long rows_off(const VitSeq& q) { return q.bp_off * 4; }          // floats

template <int SPT>
__global__ __launch_bounds__(1024) void ctc_fb_forward_kernel(const VitSeq* __restrict__ seqs, const float* __restrict__ lp, int ld, int r0,
                                                              const int* __restrict__ rows, const int* __restrict__ tokens, int blank,
                                                              float* __restrict__ alpha_all, double* __restrict__ csum,
                                                              float* __restrict__ coff, float* __restrict__ arows) {
  constexpr int NT = SPT / 2;                      // tokens per thread: local state 2k + 1 is token s0 / 2 + k, even states are blank
  __shared__ float bnd[2][1024];                   // per thread: alpha of its last state
  __shared__ float wmax[2][16];                    // per wave: maximum of the row
  const VitSeq q = seqs[blockIdx.x];
  if (q.f0 >= q.f1) return;                        // nothing of this lattice in the slab (uniform over the workgroup)
  const int tid = threadIdx.x, nw = blockDim.x >> 6;
  const int s0 = tid * SPT;
  const float NEG = -INFINITY;
  const int nvalid = min(max(q.S - s0, 0), SPT);   // states of this thread that exist
  const int* y = tokens + q.tok_off;
  const int* rw = rows + q.frame_off;
  float* alpha = alpha_all + q.alpha_off;
  const long long stride = row_stride(q);
  const bool keep = arows != nullptr && s0 + SPT <= stride;
  float* arow = keep ? arows + rows_off(q) + s0 : nullptr;

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
  auto row_of = [&](int fr) { return rw[min(fr, q.f1 - 1)] - r0; };   // past the last frame of this launch: clamped (in-bounds load)
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
    const int lo = q.S - 2 * (q.T - fr) - s0;      // the maximum runs over the states that can still reach the end
    float m = NEG;
#pragma unroll
    for (int j = 0; j < SPT; ++j) m = fmaxf(m, j >= lo ? a[j] : NEG);
    m = wave_max(m);
    if ((tid & 63) == 0) wmax[par][tid >> 6] = m;
    bnd[par][tid] = a[SPT - 1];
    __syncthreads();
  };

  int f = q.f0;
  double C = 0.0;
  fill(row_of(f));
  if (f == 0) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = NEG;
    if (tid == 0) { a[0] = eb; a[1] = et[0]; if (coff) coff[q.frame_off] = 0.f; }
    store_row(0);
    f = 1;
    fill(row_of(1));
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j) a[j] = j < nvalid ? alpha[s0 + j] : NEG;
    if (tid == 0) C = csum[blockIdx.x];
  }
  publish(f - 1);

  for (; f < q.f1; ++f) {
    const char* row = (const char*)(lp + (size_t)row_of(f + 1) * ld);
    const float left = tid > 0 ? bnd[par][tid - 1] : NEG;
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
    if (tid == 0) { C += (double)c; if (coff) coff[q.frame_off + f] = c; }
    store_row(f);
    par ^= 1;
    publish(f);
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < nvalid) alpha[s0 + j] = a[j];
  if (tid == 0) csum[blockIdx.x] = C;
}

// one lane per lattice: loglik = C[T-1] + ll^ in fp64, ll^ = logsumexp of the two end states of the last normalised row
__global__ void ctc_fb_loglik_kernel(const VitSeq* __restrict__ seqs, const float* __restrict__ alpha_all, const double* __restrict__ csum,
                                     double* __restrict__ loglik, float* __restrict__ llhat) {
  if (threadIdx.x != 0) return;
  const VitSeq q = seqs[blockIdx.x];
  const float* alpha = alpha_all + q.alpha_off;
  const double a1 = alpha[q.S - 1], a2 = alpha[q.S - 2];
  const double m = a1 > a2 ? a1 : a2;
  double l = -INFINITY;
  if (m > -INFINITY) l = m + log(exp(a1 - m) + exp(a2 - m));
  loglik[blockIdx.x] = csum[blockIdx.x] + l;
  llhat[blockIdx.x] = (float)l;
}

// per-token reductions of the posteriors, carried in HBM between launches
struct FbAcc { float* occ; float* tsum; float* peak; int* peak_frame; };

template <int SPT>
__global__ __launch_bounds__(1024) void ctc_fb_backward_kernel(const VitSeq* __restrict__ seqs, const float* __restrict__ lp, int ld, int r0,
                                                               const int* __restrict__ rows, const int* __restrict__ tokens, int blank,
                                                               float* __restrict__ beta_all, const float* __restrict__ coff,
                                                               const float* __restrict__ arows, const float* __restrict__ llhat,
                                                               float* __restrict__ zcarry, FbAcc acc) {
  constexpr int NT = SPT / 2;
  constexpr int CH = SPT < 32 ? SPT : 8;           // states whose alpha is loaded together (32 per thread: in pieces, for the registers)
  __shared__ float2 bnd[2][1024];                  // per thread: beta of its first two states (what the left neighbour's last two read)
  __shared__ float wsum[2][16];                    // per wave: sum of exp(gamma) of the row before normalisation
  const VitSeq q = seqs[blockIdx.x];
  if (q.f0 >= q.f1) return;
  const int tid = threadIdx.x, nw = blockDim.x >> 6;
  const int s0 = tid * SPT;
  const float NEG = -INFINITY;
  const int nvalid = min(max(q.S - s0, 0), SPT);
  const int* y = tokens + q.tok_off;
  const int* rw = rows + q.frame_off;
  float* beta = beta_all + q.alpha_off;
  const float* cf = coff + q.frame_off;
  const long long stride = row_stride(q);
  const bool have_row = s0 + SPT <= stride;        // else: every state of this thread lies past S - 1
  const float* arow = arows + rows_off(q) + (have_row ? s0 : 0);
  const bool first = q.f1 == q.T;                  // this launch starts the sweep at the last frame

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
  auto row_of = [&](int fr) { return rw[max(fr, q.f0)] - r0; };      // below the first frame of this launch: clamped
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
  auto step = [&](int f, bool init, float ll) {
    const char* row = (const char*)(lp + (size_t)row_of(f - 1) * ld);
    const float c = cn;
    cn = cf[f];
    float2 right = make_float2(NEG, NEG);
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
  if (first) {
#pragma unroll
    for (int k = 0; k < NT; ++k) { occ[k] = 0.f; ts[k] = 0.f; pk[k] = -1.f; pf[k] = 0; }
#pragma unroll
    for (int j = 0; j < SPT; ++j) b[j] = NEG;
    step(f, true, llhat[blockIdx.x]);
    --f;
  } else {
#pragma unroll
    for (int j = 0; j < SPT; ++j) b[j] = j < nvalid ? beta[s0 + j] : NEG;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int i = s0 / 2 + k;
      const bool have = i < q.L;
      occ[k] = have ? acc.occ[q.tok_off + i] : 0.f;
      ts[k] = have ? acc.tsum[q.tok_off + i] : 0.f;
      pk[k] = have ? acc.peak[q.tok_off + i] : -1.f;
      pf[k] = have ? acc.peak_frame[q.tok_off + i] : 0;
    }
    cn = cf[q.f1];
    // the Z the previous launch ended with, republished as wave 0's sum: adding the zeros of the other waves leaves its bits alone
    if ((tid & 63) == 0) wsum[0][tid >> 6] = tid == 0 ? zcarry[blockIdx.x] : 0.f;
    bnd[0][tid] = make_float2(b[0], b[1]);
    __syncthreads();
  }
  for (; f >= q.f0; --f) step(f, false, 0.f);

#pragma unroll
  for (int j = 0; j < SPT; ++j)
    if (j < nvalid) beta[s0 + j] = b[j];
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int i = s0 / 2 + k;
    if (i < q.L) {
      acc.occ[q.tok_off + i] = occ[k]; acc.tsum[q.tok_off + i] = ts[k];
      acc.peak[q.tok_off + i] = pk[k]; acc.peak_frame[q.tok_off + i] = pf[k];
    }
  }
  if (tid == 0) {
    float z = wsum[par][0];
    for (int w = 1; w < nw; ++w) z += wsum[par][w];
    zcarry[blockIdx.x] = z;
  }
}

}  // namespace

int ctc_fb_forward(hipStream_t s, const VitSeq* seqs, int n_seq, int max_S, const float* lp, int ld, int r0, const int* rows,
                   const int* tokens, int blank, float* alpha, double* csum, float* coff, float* arows) {
  if (n_seq <= 0) return OK;
  if (max_S < 3 || max_S > CTC_ALIGN_MAX_STATES) { set_error("ctc_fb_forward: states out of range"); return E_ARG; }
  const int spt = ctc_spt_for(max_S), threads = ctc_threads(max_S, spt);
  if (spt == 4) ctc_fb_forward_kernel<4><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, alpha, csum, coff, arows);
  else if (spt == 16) ctc_fb_forward_kernel<16><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, alpha, csum, coff, arows);
  else ctc_fb_forward_kernel<32><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, alpha, csum, coff, arows);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int ctc_fb_loglik(hipStream_t s, const VitSeq* seqs, int n_seq, const float* alpha, const double* csum, double* loglik, float* llhat) {
  if (n_seq <= 0) return OK;
  ctc_fb_loglik_kernel<<<n_seq, 64, 0, s>>>(seqs, alpha, csum, loglik, llhat);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int ctc_fb_backward(hipStream_t s, const VitSeq* seqs, int n_seq, int max_S, const float* lp, int ld, int r0, const int* rows,
                    const int* tokens, int blank, float* beta, const float* coff, const float* arows, const float* llhat, float* zcarry,
                    float* occ, float* tsum, float* peak, int* peak_frame) {
  if (n_seq <= 0) return OK;
  if (max_S < 3 || max_S > CTC_ALIGN_MAX_STATES) { set_error("ctc_fb_backward: states out of range"); return E_ARG; }
  const int spt = ctc_spt_for(max_S), threads = ctc_threads(max_S, spt);
  const FbAcc acc{occ, tsum, peak, peak_frame};
  if (spt == 4)
    ctc_fb_backward_kernel<4><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, beta, coff, arows, llhat, zcarry, acc);
  else if (spt == 16)
    ctc_fb_backward_kernel<16><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, beta, coff, arows, llhat, zcarry, acc);
  else
    ctc_fb_backward_kernel<32><<<n_seq, threads, 0, s>>>(seqs, lp, ld, r0, rows, tokens, blank, beta, coff, arows, llhat, zcarry, acc);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

// ------------------------------------------------------------------------------------ host driver (engine + lab hook)
int CtcScorer::plan(const char* who, const int32_t* tokens, const int32_t* tok_lens, int n_seq,
                    const std::vector<std::vector<int32_t>>& seq_rows, int V, int blank_id) {
  return lat.plan(who, tokens, tok_lens, n_seq, seq_rows, V, blank_id);
}

int CtcScorer::begin(hipStream_t s, bool posteriors) {
  post = posteriors;
  const size_t n_seq = lat.seq.size(), n_tok = lat.h_tokens.size();
  RVB_TRY(lat.d_tokens.ensure(n_tok * 4));
  RVB_TRY(lat.d_rows.ensure(lat.h_rows.size() * 4));
  RVB_TRY(lat.d_seqs.ensure(n_seq * sizeof(VitSeq)));
  RVB_TRY(lat.d_alpha.ensure(lat.alpha_floats * 4));
  RVB_TRY(d_csum.ensure(n_seq * 8));
  RVB_TRY(d_loglik.ensure(n_seq * 8));
  RVB_TRY(d_llhat.ensure(n_seq * 4));
  if (post) {
    const size_t row_bytes = lat.bp_bytes * 16;    // the layout of the 2-bit back-pointers at 4 bytes per frame and state
    const std::string what = "ctc score: " + std::to_string(row_bytes) + " bytes of alpha rows (4 bytes per frame and state) do not fit: ";
    // lab hook (librvb_test.so only): pretend that more than RVB_CTC_SCORE_FAKE_NOMEM_ABOVE bytes of alpha rows do not fit
    if (const char* f = lab_env("RVB_CTC_SCORE_FAKE_NOMEM_ABOVE")) {
      if ((double)row_bytes > atof(f)) { set_error(what + "hipMalloc refused (RVB_CTC_SCORE_FAKE_NOMEM_ABOVE)"); return E_NOMEM; }
    }
    if (int r = d_arows.ensure(row_bytes)) { set_error(what + last_error()); return r; }
    RVB_TRY(d_coff.ensure((size_t)lat.total_frames * 4));
    RVB_TRY(d_beta.ensure(lat.alpha_floats * 4));
    RVB_TRY(d_z.ensure(n_seq * 4));
    RVB_TRY(d_acc.ensure(n_tok * 16));
  }
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_tokens.p, lat.h_tokens.data(), n_tok * 4, hipMemcpyHostToDevice, s));
  RVB_HIP_CHECK(hipMemcpyAsync(lat.d_rows.p, lat.h_rows.data(), lat.h_rows.size() * 4, hipMemcpyHostToDevice, s));
  for (auto& q : lat.seq) q.f0 = q.f1 = 0;
  return OK;
}

int CtcScorer::advance(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  bool any;
  RVB_TRY(slab_window("ctc score", false, lat.seq, lat.h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, lat.d_seqs.p, lat.seq));
  return ctc_fb_forward(s, lat.d_seqs.as<VitSeq>(), (int)lat.seq.size(), lat.max_S, lp, ld, r0, lat.d_rows.as<int>(), lat.d_tokens.as<int>(),
                        lat.blank, lat.d_alpha.as<float>(), d_csum.as<double>(), post ? d_coff.as<float>() : nullptr,
                        post ? d_arows.as<float>() : nullptr);
}

int CtcScorer::finish_forward(hipStream_t s, double* loglik) {
  RVB_TRY(slab_covered("ctc score", false, lat.seq));
  for (auto& q : lat.seq) q.f0 = q.f1 = q.T;       // the backward sweep starts above the last frame
  RVB_TRY(ctc_fb_loglik(s, lat.d_seqs.as<VitSeq>(), (int)lat.seq.size(), lat.d_alpha.as<float>(), d_csum.as<double>(), d_loglik.as<double>(),
                         d_llhat.as<float>()));
  RVB_HIP_CHECK(hipMemcpyAsync(loglik, d_loglik.p, lat.seq.size() * 8, hipMemcpyDeviceToHost, s));
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  return slab_feasible("ctc score", lat.seq, loglik, "emits the transcript");
}

int CtcScorer::advance_backward(hipStream_t s, const float* lp, int ld, int r0, int nrows) {
  if (!post) { set_error("ctc score: backward sweep without alpha rows"); return E_STATE; }
  bool any;
  RVB_TRY(slab_window("ctc score", true, lat.seq, lat.h_rows, r0, nrows, &any));
  if (!any) return OK;
  RVB_TRY(slab_upload(s, lat.d_seqs.p, lat.seq));
  float* acc = d_acc.as<float>();
  const size_t n_tok = lat.h_tokens.size();
  return ctc_fb_backward(s, lat.d_seqs.as<VitSeq>(), (int)lat.seq.size(), lat.max_S, lp, ld, r0, lat.d_rows.as<int>(), lat.d_tokens.as<int>(),
                         lat.blank, d_beta.as<float>(), d_coff.as<float>(), d_arows.as<float>(), d_llhat.as<float>(), d_z.as<float>(), acc,
                         acc + n_tok, acc + 2 * n_tok, (int*)(acc + 3 * n_tok));
}

int CtcScorer::finish_backward(hipStream_t s, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  RVB_TRY(slab_covered("ctc score", true, lat.seq));
  const size_t n_tok = lat.h_tokens.size();
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

void CtcScorer::release() {
  lat.release();
  for (DevBuf* b : {&d_csum, &d_loglik, &d_llhat, &d_coff, &d_arows, &d_beta, &d_z, &d_acc}) b->release();
}

}  // namespace rvb
