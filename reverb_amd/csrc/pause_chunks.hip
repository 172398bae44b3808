// Chunks cut at pauses (rvb_pause_chunks; the definition is stated once, in include/rvb.h).
//
// The reference cuts a recording every chunk_size frames wherever the clock says (feats_batcher, cli/reverb.py:148-180).  Here the
// cut may fall anywhere in the `search` frames before that boundary, at the quietest place: the minimum of the loudness e (sum of a
// frame's 80 log-mel values) summed over 2h frames around the cut.  Three small kernels over the features that are resident anyway:
//   pause_loudness  e per live frame; 4 lanes per row, five 128-bit loads each (reads the features once: 320 B per frame)
//   pause_cuts      one workgroup per recording, serial over its pieces: the window's e staged in LDS, one candidate per thread, a
//                   wave64 (value, index) arg-min with the last-minimum and NaN rules (reads <= search + 2h floats per piece)
//   pause_gather    piece k's rows to chunk slot k of a second buffer, 128-bit copies, the slot's tail zeroed (reads the live rows
//                   once, writes chunks * chunk_size rows)
// No running or prefix sums: e is ONE sum of 80 terms and s ONE sum of 2h values of e, which is what the tests' error bound assumes.
#include "pause_chunks.h"

#include <algorithm>
#include <string>
#include <vector>

#include "engine_impl.h"

namespace rvb {

static constexpr int NMEL = 80, ROW_V4 = NMEL / 4;      // a feature row is 20 float4
static constexpr int CUT_TILE = 1024;                   // candidates per LDS tile of the cut search

__global__ __launch_bounds__(256) void pause_loudness_kernel(const float* __restrict__ feats, const int64_t* __restrict__ frame0,
                                                             const PauseRec* __restrict__ rec, int n_rec, float* __restrict__ loud) {
  const int64_t frame = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);     // 4 lanes per frame, 64 frames per workgroup
  const int q = threadIdx.x & 3;
  const bool live = frame < frame0[n_rec];       // the same for the 4 lanes of a frame
  float acc = 0.f;
  int64_t row = 0;
  if (live) {
    int lo = 0, hi = n_rec;                      // frame0[lo] <= frame < frame0[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (frame0[mid] <= frame) lo = mid; else hi = mid;
    }
    row = rec[lo].row0 + (frame - frame0[lo]);
    const float4* p = reinterpret_cast<const float4*>(feats + row * NMEL);
#pragma unroll
    for (int i = 0; i < ROW_V4 / 4; ++i) {
      const float4 v = p[q + 4 * i];
      acc += (v.x + v.y) + (v.z + v.w);
    }
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  if (live && q == 0) loud[row] = acc;
}

// (v, c) replaces the best so far (bv, bi; bi < 0: none yet): never a NaN, the smaller value, the later position on a tie
__device__ __forceinline__ void take_min(float v, int c, float& bv, int& bi) {
  if (v == v && (bi < 0 || v < bv || (v == bv && c > bi))) { bv = v; bi = c; }
}

__global__ __launch_bounds__(256) void pause_cuts_kernel(const float* __restrict__ loud, const PauseRec* __restrict__ rec, int chunk_size,
                                                         int search, int h, int32_t* __restrict__ table, int32_t* __restrict__ count) {
  __shared__ float s_e[CUT_TILE + 2 * PAUSE_MAX_SMOOTH];
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  __shared__ int s_cut;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const PauseRec r = rec[blockIdx.x];
  const int n = r.n_frames;
  const float* e = loud + r.row0;
  int32_t* tab = table + r.tab0;
  if (n <= 0) {
    if (tid == 0) count[blockIdx.x] = 0;
    return;
  }
  if (tid == 0 && r.tab_cap > 0) tab[0] = 0;
  int start = 0, k = 0;
  while (n - start > chunk_size) {             // uniform over the workgroup
    const int lo = start + chunk_size - search;
    const int hi = min(start + chunk_size, n - 7);
    float bv = 0.f;
    int bi = -1;
    for (int c0 = lo; c0 <= hi; c0 += CUT_TILE) {
      const int c1 = min(c0 + CUT_TILE - 1, hi);
      const int m = c1 - c0 + 2 * h;           // e of the frames c0 - h .. c1 + h - 1, clamped into the recording
      __syncthreads();
      for (int i = tid; i < m; i += 256) s_e[i] = e[min(max(c0 - h + i, 0), n - 1)];
      __syncthreads();
      for (int c = c0 + tid; c <= c1; c += 256) {
        const float* win = s_e + (c - c0);
        float s = 0.f;
        for (int j = 0; j < 2 * h; ++j) s += win[j];
        take_min(s, c, bv, bi);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0) take_min(ov, oi, bv, bi);
    }
    if (lane == 0) { s_v[w] = bv; s_i[w] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int x = 1; x < 4; ++x)
        if (s_i[x] >= 0) take_min(s_v[x], s_i[x], bv, bi);
      const int cut = bi < 0 ? hi : bi;        // every candidate NaN: the latest cut
      if (k + 1 < r.tab_cap) tab[k + 1] = cut;
      s_cut = cut;
    }
    __syncthreads();
    start = s_cut;
    ++k;
  }
  if (tid == 0) count[blockIdx.x] = k + 1;
}

__global__ __launch_bounds__(256) void pause_gather_kernel(const float* __restrict__ feats, const PausePiece* __restrict__ pieces,
                                                           int chunk_size, int blocks_per_piece, float* __restrict__ out) {
  const int64_t k = blockIdx.x / blocks_per_piece;
  const int q = (blockIdx.x % blocks_per_piece) * 256 + threadIdx.x;      // float4 within the chunk slot
  if (q >= chunk_size * ROW_V4) return;
  const PausePiece p = pieces[k];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q / ROW_V4 < p.len) v = reinterpret_cast<const float4*>(feats + p.src * NMEL)[q];
  reinterpret_cast<float4*>(out + k * chunk_size * NMEL)[q] = v;
}

int pause_loudness(hipStream_t s, const float* feats, const int64_t* frame0, const PauseRec* rec, int n_rec, int64_t total_frames,
                   float* loud) {
  if (total_frames <= 0 || n_rec <= 0) return OK;
  hipLaunchKernelGGL(pause_loudness_kernel, dim3(cdiv(total_frames, 64)), dim3(256), 0, s, feats, frame0, rec, n_rec, loud);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int pause_cuts(hipStream_t s, const float* loud, const PauseRec* rec, int n_rec, int chunk_size, int search, int h, int32_t* table,
               int32_t* count) {
  if (n_rec <= 0) return OK;
  hipLaunchKernelGGL(pause_cuts_kernel, dim3(n_rec), dim3(256), 0, s, loud, rec, chunk_size, search, h, table, count);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int pause_gather(hipStream_t s, const float* feats, const PausePiece* pieces, int64_t n_pieces, int chunk_size, float* out) {
  if (n_pieces <= 0) return OK;
  const int bpp = cdiv((int64_t)chunk_size * ROW_V4, 256);
  if (n_pieces * bpp > 0x7fffffffLL) { set_error("pause_gather: too many chunks for one launch"); return E_UNSUPPORTED; }
  hipLaunchKernelGGL(pause_gather_kernel, dim3((unsigned)(n_pieces * bpp)), dim3(256), 0, s, feats, pieces, chunk_size, bpp, out);
  RVB_HIP_CHECK(hipGetLastError());
  return OK;
}

int pause_check_args(const char* who, int chunk_size, int search, int h) {
  const std::string w(who);
  if (h < 1 || h > PAUSE_MAX_SMOOTH) {
    set_error(w + ": h = " + std::to_string(h) + " (the smoothing half-width) must be in [1, " + std::to_string(PAUSE_MAX_SMOOTH) + "]");
    return E_ARG;
  }
  if (chunk_size < 7) { set_error(w + ": chunk_size must be at least 7 frames"); return E_ARG; }
  if (search < 7 || search > chunk_size - 7) {
    set_error(w + ": search = " + std::to_string(search) + " must be in [7, chunk_size - 7 = " + std::to_string(chunk_size - 7) + "]");
    return E_ARG;
  }
  return OK;
}

// the ensure() of a buffer of this call: its failure names the call (and, from DevBuf::ensure, the bytes)
static int ensure_named(DevBuf& b, size_t bytes) {
  const int r = b.ensure(bytes);
  if (r != OK) set_error(std::string("rvb_pause_chunks: ") + last_error());
  return r;
}

}  // namespace rvb

using namespace rvb;

extern "C" int rvb_fixed_chunks(rvb_engine* e) {
  if (!e) { set_error("rvb_fixed_chunks: null engine"); return E_ARG; }
  e->packed = false;
  return OK;
}

extern "C" int rvb_pause_chunks(rvb_engine* e, int chunk_size, int search, int h, int64_t* first_chunk, int32_t* starts, int32_t* lens,
                                int64_t capacity, int64_t* n_chunks, float* feats_out) {
  // every refusal of an argument comes before the engine is touched
  RVB_TRY(pause_check_args("rvb_pause_chunks", chunk_size, search, h));
  if (!e) { set_error("rvb_pause_chunks: null engine"); return E_ARG; }
  if (!first_chunk || !n_chunks) { set_error("rvb_pause_chunks: null argument (first_chunk and n_chunks are needed)"); return E_ARG; }
  if (chunk_size > e->cfg.chunk_frames) {
    set_error("rvb_pause_chunks: chunk_size " + std::to_string(chunk_size) + " exceeds the engine's chunk_frames " + std::to_string(e->cfg.chunk_frames));
    return E_ARG;
  }
  if (e->feat_kind == 0 || !e->feats.p) {
    set_error("rvb_pause_chunks: no features are resident: call rvb_fbank or rvb_fbank_batch first"); return E_STATE;
  }
  RVB_HIP_CHECK(hipSetDevice(e->device));

  // the recordings behind the resident features
  const int n_rec = e->feat_kind == 2 ? (int)e->h_rec.size() : 1;
  std::vector<PauseRec> rec(n_rec);
  std::vector<int64_t> frame0(n_rec + 1, 0);
  int64_t tab = 0;
  for (int r = 0; r < n_rec; ++r) {
    const int64_t n = e->feat_kind == 2 ? e->h_frame0[r + 1] - e->h_frame0[r] : e->n_frames;
    if (n > (1 << 30)) { set_error("rvb_pause_chunks: recording " + std::to_string(r) + " has more than 2^30 frames"); return E_UNSUPPORTED; }
    const int64_t cap = pause_max_pieces(n, chunk_size, search);
    rec[r] = PauseRec{e->feat_kind == 2 ? e->h_rec[r].row0 : 0, tab, (int32_t)n, (int32_t)cap};
    frame0[r + 1] = frame0[r] + n;
    tab += cap;
  }
  RVB_TRY(ensure_named(e->pc_loud, (size_t)std::max<int64_t>(e->feat_rows, 1) * 4));
  RVB_TRY(ensure_named(e->pc_rec, rec.size() * sizeof(PauseRec)));
  RVB_TRY(ensure_named(e->pc_frame0, frame0.size() * 8));
  RVB_TRY(ensure_named(e->pc_table, (size_t)std::max<int64_t>(tab, 1) * 4));
  RVB_TRY(ensure_named(e->pc_count, (size_t)n_rec * 4));

  Scope sc(e, "pause_chunks");
  RVB_HIP_CHECK(hipMemcpyAsync(e->pc_rec.p, rec.data(), rec.size() * sizeof(PauseRec), hipMemcpyHostToDevice, e->stream));
  RVB_HIP_CHECK(hipMemcpyAsync(e->pc_frame0.p, frame0.data(), frame0.size() * 8, hipMemcpyHostToDevice, e->stream));
  RVB_TRY(pause_loudness(e->stream, e->feats.as<float>(), e->pc_frame0.as<int64_t>(), e->pc_rec.as<PauseRec>(), n_rec, frame0[n_rec],
                         e->pc_loud.as<float>()));
  RVB_TRY(pause_cuts(e->stream, e->pc_loud.as<float>(), e->pc_rec.as<PauseRec>(), n_rec, chunk_size, search, h, e->pc_table.as<int32_t>(),
                     e->pc_count.as<int32_t>()));
  std::vector<int32_t> table((size_t)std::max<int64_t>(tab, 1)), count(n_rec);
  if (tab) RVB_HIP_CHECK(hipMemcpyAsync(table.data(), e->pc_table.p, (size_t)tab * 4, hipMemcpyDeviceToHost, e->stream));
  RVB_HIP_CHECK(hipMemcpyAsync(count.data(), e->pc_count.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost, e->stream));
  RVB_HIP_CHECK(hipStreamSynchronize(e->stream));

  // pieces of all recordings, numbered consecutively in recording order
  int64_t total = 0;
  for (int r = 0; r < n_rec; ++r) {
    if (count[r] < 0 || count[r] > rec[r].tab_cap) { set_error("rvb_pause_chunks: the cut search left its table (internal error)"); return E_HIP; }
    total += count[r];
  }
  if (total > capacity || (total && (!starts || !lens))) {
    *n_chunks = total;
    set_error("rvb_pause_chunks: capacity " + std::to_string(capacity) + " is too small: the cuts give " + std::to_string(total) + " chunks");
    return E_ARG;
  }
  std::vector<PausePiece> pieces((size_t)total);
  int64_t k = 0;
  for (int r = 0; r < n_rec; ++r)
    for (int j = 0; j < count[r]; ++j, ++k) {
      const int32_t s0 = table[rec[r].tab0 + j];
      const int32_t s1 = j + 1 < count[r] ? table[rec[r].tab0 + j + 1] : rec[r].n_frames;
      if (s0 < 0 || s1 <= s0 || s1 - s0 > chunk_size || s1 > rec[r].n_frames) {
        set_error("rvb_pause_chunks: the cut search gave a piece outside its recording (internal error)"); return E_HIP;
      }
      pieces[k] = PausePiece{rec[r].row0 + s0, s1 - s0, 0};
    }
  const int64_t rows = total * chunk_size;
  RVB_TRY(ensure_named(e->feats_packed, (size_t)std::max<int64_t>(rows, 1) * NMEL * 4));
  RVB_TRY(ensure_named(e->pc_pieces, std::max<size_t>(pieces.size(), 1) * sizeof(PausePiece)));
  if (total) {
    RVB_HIP_CHECK(hipMemcpyAsync(e->pc_pieces.p, pieces.data(), pieces.size() * sizeof(PausePiece), hipMemcpyHostToDevice, e->stream));
    RVB_TRY(pause_gather(e->stream, e->feats.as<float>(), e->pc_pieces.as<PausePiece>(), total, chunk_size, e->feats_packed.as<float>()));
    if (feats_out) RVB_HIP_CHECK(hipMemcpyAsync(feats_out, e->feats_packed.p, (size_t)rows * NMEL * 4, hipMemcpyDeviceToHost, e->stream));
    RVB_HIP_CHECK(hipStreamSynchronize(e->stream));       // `pieces` is free from here on
  }
  k = 0;
  for (int r = 0; r < n_rec; ++r) {
    first_chunk[r] = k;
    for (int j = 0; j < count[r]; ++j, ++k) {
      starts[k] = table[rec[r].tab0 + j];
      lens[k] = pieces[k].len;
    }
  }
  first_chunk[n_rec] = total;
  *n_chunks = total;
  e->packed = true; e->packed_rows = rows;
  return OK;
}
