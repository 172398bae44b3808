// rvb_test_*: raw kernel entry points used by tests/ (host buffers in, host buffers out).  Each one
// uploads fp32 host data (rounded to the compute dtype with the same RNE conversion the engine
// uses), launches exactly the kernel the engine launches, and downloads the result as fp32.
#include "mp3.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "test_api.h"
#include "engine_impl.h"
#include "kernels.h"
#include "search.h"
#include "trie.h"

using namespace rvb;

namespace rvb {
const char* lab_env(const char* name) { return getenv(name); }      // librvb_test.so: the lab build reads its switches (librvb.so: lab_env_off.cpp)
}

namespace {
struct Dev {
  void* p = nullptr;
  ~Dev() { if (p) (void)hipFree(p); }
  int alloc(size_t n) { if (n == 0) n = 16; if (hipMalloc(&p, n) != hipSuccess) { set_error("hipMalloc failed in test api"); return E_NOMEM; } return OK; }
};
int up_T(Dev& d, int dtype, const float* src, size_t n) {
  if (!src) return OK;
  int r = d.alloc(n * dt_size(dtype));
  if (r != OK) return r;
  if (dtype == DT_F32) { RVB_HIP_CHECK(hipMemcpy(d.p, src, n * 4, hipMemcpyHostToDevice)); return OK; }
  std::vector<bf16_t> t(n);
  for (size_t i = 0; i < n; ++i) t[i] = f32_to_bf16(src[i]);
  RVB_HIP_CHECK(hipMemcpy(d.p, t.data(), n * 2, hipMemcpyHostToDevice));
  return OK;
}
int up_raw(Dev& d, const void* src, size_t bytes) {
  if (!src) return OK;
  int r = d.alloc(bytes);
  if (r != OK) return r;
  RVB_HIP_CHECK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return OK;
}
int down_T(const Dev& d, int dtype, bool as_f32, float* dst, size_t n) {
  if (dtype == DT_F32 || as_f32) { RVB_HIP_CHECK(hipMemcpy(dst, d.p, n * 4, hipMemcpyDeviceToHost)); return OK; }
  std::vector<bf16_t> t(n);
  RVB_HIP_CHECK(hipMemcpy(t.data(), d.p, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) dst[i] = bf16_to_f32(t[i]);
  return OK;
}
int need_gpu() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device available: librvb has no CPU fallback"); return E_HIP; }
  return OK;
}
// the frame rows of n_seq lattices whose frames lie back to back: rows[i][t] = (frames before lattice i) + t.  A count over the cap
// keeps its size and gets no values: plan() refuses it on the count alone.  -> the rows in all
int64_t lab_rows(const int32_t* T, int n_seq, std::vector<std::vector<int32_t>>* rows) {
  rows->assign(n_seq, {});
  int64_t total = 0;
  for (int i = 0; i < n_seq; ++i) {
    (*rows)[i].resize((size_t)T[i]);
    if (T[i] <= CTC_ALIGN_MAX_FRAMES) for (int t = 0; t < T[i]; ++t) (*rows)[i][t] = (int32_t)(total + t);
    total += T[i];
  }
  return total;
}
// feeds M rows to advance(r0, nrows), slab_rows at a time, for as long as r stays OK: ascending from row 0, or descending in slabs
// that END at the last row, so that the two sweeps of the scorer cut at different frames
template <typename F> int feed_slabs(int r, int64_t M, int slab_rows, bool descending, F advance) {
  for (int64_t done = 0; r == OK && done < M; done += slab_rows) {
    const int n = (int)std::min<int64_t>(slab_rows, M - done);
    r = advance((int)(descending ? M - done - n : done), n);
  }
  return r;
}
// the lab run of either aligner over M rows of host log-probs (w: their maxima, null without wildcards): upload, begin, the slabs,
// the back-trace into states [M] and score [sequences]; the aligner's buffers are released whatever happens
template <typename Aligner>
int lab_align(Aligner& al, const float* lp, const float* w, int64_t M, int V, int slab_rows, float bias, std::vector<int32_t>* states,
              float* score) {
  RVB_TRY(need_gpu());
  Dev dlp, dw;
  int r = up_raw(dlp, lp, (size_t)M * V * 4);
  if (r == OK) r = up_raw(dw, w, (size_t)M * 4);
  if (r == OK) r = al.begin(nullptr);
  r = feed_slabs(r, M, slab_rows, false, [&](int r0, int n) {
    return al.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n, w ? (const float*)dw.p + r0 : nullptr, bias);
  });
  states->resize((size_t)M);
  if (r == OK) r = al.finish(nullptr, states->data(), score);
  if (r != OK) (void)hipDeviceSynchronize();
  al.release();
  return r;
}
}  // namespace

extern "C" {

int rvb_test_gemm(int dtype, const float* A, const float* W, const float* bias, const float* res, float* C, int M,
                  int N, int K, float alpha, int act, int out_f32, int conv, int cT1, int cF1, int cC, int cB) {
  RVB_TRY(need_gpu());
  Dev dA, dW, dB, dR, dC;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  size_t a_elems = (size_t)M * K;
  if (conv) {
    const int T2 = (cT1 - 3) / 2 + 1, F2 = (cF1 - 3) / 2 + 1;
    if (M != cB * T2 * F2 || K != 9 * cC) { set_error("rvb_test_gemm: conv shape mismatch"); return E_ARG; }
    a_elems = (size_t)cB * cT1 * cF1 * cC;
    g.conv = 1; g.cT1 = cT1; g.cF1 = cF1; g.cT2 = T2; g.cF2 = F2; g.cC = cC;
  }
  RVB_TRY(up_T(dA, dtype, A, a_elems));
  RVB_TRY(up_T(dW, dtype, W, (size_t)N * K));
  RVB_TRY(up_raw(dB, bias, (size_t)N * 4));
  RVB_TRY(up_raw(dR, res, (size_t)M * N * 4));
  const bool f32out = dtype == DT_F32 || out_f32;
  RVB_TRY(dC.alloc((size_t)M * N * (f32out ? 4 : 2)));
  g.A = dA.p; g.W = dW.p; g.bias = (const float*)dB.p; g.res = (const float*)dR.p; g.C = dC.p;
  g.M = M; g.N = N; g.K = K; g.lda = conv ? cC : K; g.ldw = K; g.ldc = N; g.ldres = N;
  g.alpha = alpha; g.act = act; g.out_f32 = out_f32;
  RVB_TRY(gemm(nullptr, dtype, g));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dC, dtype, f32out, C, (size_t)M * N);
}

int rvb_test_gemm_rowadd(const float* A, const float* W, const float* bias, const float* add, float* C, int M, int N, int K,
                         int add_rows, int add_col0, int add_cols) {
  RVB_TRY(need_gpu());
  Dev dA, dW, dB, dP, dC;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  RVB_TRY(up_T(dA, DT_BF16, A, (size_t)M * K));
  RVB_TRY(up_T(dW, DT_BF16, W, (size_t)N * K));
  RVB_TRY(up_raw(dB, bias, (size_t)N * 4));
  RVB_TRY(up_T(dP, DT_BF16, add, (size_t)add_rows * add_cols));
  RVB_TRY(dC.alloc((size_t)M * N * 2));
  g.A = dA.p; g.W = dW.p; g.bias = (const float*)dB.p; g.C = dC.p;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N; g.alpha = 1.f; g.act = ACT_NONE;
  g.rowadd = dP.p; g.rowadd_rows = add_rows; g.rowadd_ld = add_cols; g.rowadd_col0 = add_col0; g.rowadd_cols = add_cols;
  RVB_TRY(gemm(nullptr, DT_BF16, g));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dC, DT_BF16, false, C, (size_t)M * N);
}

// bf16 GEMM with the ACT_GLU epilogue: W rows / bias / output columns interleaved as the engine packs them (row 2c = a_c, 2c + 1 = b_c);
// C [M, N / 2] = a * sigmoid(b)
int rvb_test_gemm_glu(const float* A, const float* W, const float* bias, float* C, int M, int N, int K) {
  RVB_TRY(need_gpu());
  Dev dA, dW, dB, dC;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  RVB_TRY(up_T(dA, DT_BF16, A, (size_t)M * K));
  RVB_TRY(up_T(dW, DT_BF16, W, (size_t)N * K));
  RVB_TRY(up_raw(dB, bias, (size_t)N * 4));
  RVB_TRY(dC.alloc((size_t)M * (N / 2) * 2));
  g.A = dA.p; g.W = dW.p; g.bias = (const float*)dB.p; g.C = dC.p;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N / 2; g.alpha = 1.f; g.act = ACT_GLU;
  if (!gemm_glu_supported(DT_BF16, g)) { set_error("rvb_test_gemm_glu: shape not supported by the ACT_GLU epilogue"); return E_UNSUPPORTED; }
  RVB_TRY(gemm(nullptr, DT_BF16, g));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dC, DT_BF16, false, C, (size_t)M * (N / 2));
}

int64_t rvb_test_mp3_decode(const void* data, int64_t nbytes, int channel, float* out, int64_t capacity, int64_t* info9, int64_t* stats12, int threads) {
  try {
    rvb::mp3::Info i;
    rvb::mp3::Stats st;
    const int64_t r = rvb::mp3::decode((const uint8_t*)data, (size_t)nbytes, channel, out, capacity, &i, &st, threads);
    if (info9) { info9[0] = i.version; info9[1] = i.channels; info9[2] = i.sample_rate; info9[3] = i.audio_frames; info9[4] = i.samples_per_frame;
                 info9[5] = i.has_info_frame; info9[6] = i.start_skip; info9[7] = i.samples; info9[8] = i.bitrate_kbps; }
    if (stats12) { stats12[0] = st.granules; stats12[1] = st.huff_exact; stats12[2] = st.huff_short; stats12[3] = st.huff_overrun; stats12[4] = st.crc_checked;
                   stats12[5] = st.crc_failed; stats12[6] = st.reservoir_missing; stats12[7] = st.short_granules; stats12[8] = st.mixed_granules;
                   stats12[9] = st.ms_granules; stats12[10] = st.intensity_granules; stats12[11] = st.max_main_data_begin; }
    return r;
  } catch (const rvb::mp3::Error& e) {
    set_error(e.msg);
    return e.code;
  }
}
int rvb_test_mp3_hybrid(float* xr, float* overlap, int block_type, int mixed, float* out) { rvb::mp3::hybrid_granule(xr, overlap, block_type, mixed, 2, out); return OK; }
int rvb_test_mp3_polyphase(const float* sb, float* vbuf, int* voff, float* pcm) { rvb::mp3::polyphase_granule(sb, vbuf, voff, pcm); return OK; }
int rvb_test_mp3_window(float* out512) { memcpy(out512, rvb::mp3::synthesis_window(), 512 * sizeof(float)); return OK; }
int rvb_test_mp3_huffman(int t, uint16_t* codes, uint8_t* lens, int32_t* linbits32) {
  const uint16_t* c = nullptr; const uint8_t* l = nullptr;
  int lb[32];
  const int n = rvb::mp3::huffman_table(t, &c, &l, lb);
  if (linbits32) for (int i = 0; i < 32; ++i) linbits32[i] = lb[i];
  if (n > 0) { memcpy(codes, c, 2 * (size_t)n); memcpy(lens, l, (size_t)n); }
  return n;
}

int rvb_test_rownorm(int dtype, const float* x, const float* gamma, const float* beta, float eps, int mode, int silu,
                     const float* add, float* out, int out_f32, int M, int d) {
  RVB_TRY(need_gpu());
  Dev dx, dg, db, da, dout;
  const bool x16 = (mode & 256) != 0;            // bit 8 of `mode`: x is handed to the kernel as bf16 (bf16 engine, conv-module norm)
  mode &= 255;
  if (x16) RVB_TRY(up_T(dx, DT_BF16, x, (size_t)M * d)); else RVB_TRY(up_raw(dx, x, (size_t)M * d * 4));
  RVB_TRY(up_raw(dg, gamma, (size_t)d * 4));
  RVB_TRY(up_raw(db, beta, (size_t)d * 4));
  RVB_TRY(up_T(da, dtype, add, (size_t)M * d));
  const bool f32out = dtype == DT_F32 || out_f32;
  RVB_TRY(dout.alloc((size_t)M * d * (f32out ? 4 : 2)));
  NormArgs a;
  a.x = (const float*)dx.p; a.gamma = (const float*)dg.p; a.beta = (const float*)db.p; a.eps = eps; a.mode = mode;
  a.silu = silu; a.add = da.p; a.out = dout.p; a.out_f32 = out_f32; a.M = M; a.d = d;
  a.x_bf16 = x16 ? 1 : 0;
  RVB_TRY(rownorm(nullptr, dtype, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, f32out, out, (size_t)M * d);
}

int rvb_test_conv1(int dtype, const float* feats, const float* mean, const float* istd, const float* w, const float* b,
                   float* out, int B, int T0, int F0, int d) {
  RVB_TRY(need_gpu());
  const int T1 = (T0 - 3) / 2 + 1, F1 = (F0 - 3) / 2 + 1;
  Dev df, dm, di, dw, db, dout;
  RVB_TRY(up_raw(df, feats, (size_t)B * T0 * F0 * 4));
  RVB_TRY(up_raw(dm, mean, (size_t)F0 * 4));
  RVB_TRY(up_raw(di, istd, (size_t)F0 * 4));
  std::vector<float> wt((size_t)d * 9);            // the caller passes conv.0.weight as the reference stores it, [d][1][3][3]
  for (int c = 0; c < d; ++c)
    for (int k = 0; k < 9; ++k) wt[(size_t)k * d + c] = w[(size_t)c * 9 + k];
  RVB_TRY(up_raw(dw, wt.data(), (size_t)d * 9 * 4));
  RVB_TRY(up_raw(db, b, (size_t)d * 4));
  const size_t n = (size_t)B * T1 * F1 * d;
  RVB_TRY(dout.alloc(n * dt_size(dtype)));
  RVB_TRY(subsample_conv1(nullptr, dtype, (const float*)df.p, (const float*)dm.p, (const float*)di.p, (const float*)dw.p,
                        (const float*)db.p, dout.p, B, T0, F0, d));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, false, out, n);
}

// conv_block.hip on host floats: x [B][F][T][32] (unbordered NHWC), wa / wb [32][32][3][3] as torch stores Conv2d weights (BatchNorm
// already folded by the caller), ba / bb [32]; out [B][F][T][32].  Builds the bordered planes and conv2d's weight layout.
int rvb_test_conv_block32(const float* x, const float* wa, const float* ba, const float* wb, const float* bb, float* out, int B, int F, int T) {
  RVB_TRY(need_gpu());
  if (!x || !wa || !ba || !wb || !bb || !out || B < 1 || F < 1 || T < 1) { set_error("rvb_test_conv_block32: bad argument"); return E_ARG; }
  const int FP = F + 2, TP = T + 2;
  const size_t np = (size_t)B * FP * TP * 32;
  std::vector<bf16_t> xb(np, 0);
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < F; ++f)
      for (int t = 0; t < T; ++t)
        for (int c = 0; c < 32; ++c) xb[(((size_t)b * FP + f + 1) * TP + t + 1) * 32 + c] = f32_to_bf16(x[(((size_t)b * F + f) * T + t) * 32 + c]);
  auto pack_w = [](const float* w) {                 // [o][ci][kh][kw] -> [tap][1][o][ci]
    std::vector<bf16_t> p((size_t)9 * 32 * 32);
    for (int o = 0; o < 32; ++o)
      for (int ci = 0; ci < 32; ++ci)
        for (int t = 0; t < 9; ++t) p[((size_t)t * 32 + o) * 32 + ci] = f32_to_bf16(w[((size_t)o * 32 + ci) * 9 + t]);
    return p;
  };
  const std::vector<bf16_t> pa = pack_w(wa), pb = pack_w(wb);
  Dev dx, dwa, dwb, dba, dbb, dout;
  RVB_TRY(up_raw(dx, xb.data(), np * 2)); RVB_TRY(up_raw(dwa, pa.data(), pa.size() * 2)); RVB_TRY(up_raw(dwb, pb.data(), pb.size() * 2));
  RVB_TRY(up_raw(dba, ba, 32 * 4)); RVB_TRY(up_raw(dbb, bb, 32 * 4));
  RVB_TRY(dout.alloc(np * 2 + 256)); RVB_HIP_CHECK(hipMemset(dout.p, 0, np * 2 + 256));
  if (!conv_block32_applicable(DT_BF16, 32, 32, 32, 1, 1, 9, 9, F, T)) { set_error("rvb_test_conv_block32: the fused block is switched off (RVD_CONV_BLOCK=0)"); return E_STATE; }
  ConvBlockArgs a{};
  a.in = dx.p; a.wa = dwa.p; a.ba = (const float*)dba.p; a.wb = dwb.p; a.bb = (const float*)dbb.p; a.out = dout.p; a.B = B; a.F = F; a.T = T;
  RVB_TRY(conv_block32(nullptr, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  std::vector<bf16_t> ob(np);
  RVB_HIP_CHECK(hipMemcpy(ob.data(), dout.p, np * 2, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < F; ++f)
      for (int t = 0; t < T; ++t)
        for (int c = 0; c < 32; ++c) out[(((size_t)b * F + f) * T + t) * 32 + c] = bf16_to_f32(ob[(((size_t)b * FP + f + 1) * TP + t + 1) * 32 + c]);
  // the zero border of the output plane must be untouched (the next convolution relies on it)
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < FP; ++f)
      for (int t = 0; t < TP; ++t)
        if (f == 0 || f == FP - 1 || t == 0 || t == TP - 1)
          for (int c = 0; c < 32; ++c)
            if (ob[(((size_t)b * FP + f) * TP + t) * 32 + c] != 0) { set_error("rvb_test_conv_block32: the kernel wrote into the zero border"); return E_STATE; }
  return OK;
}

int rvb_test_conv_s2sc(const float* x, const float* w, const float* b, const float* wsc, const float* bsc, float* out, float* sc, int B, int Fi, int Ti) {
  RVB_TRY(need_gpu());
  if (!x || !w || !b || !wsc || !bsc || !out || !sc || B < 1 || Fi < 1 || Ti < 1) { set_error("rvb_test_conv_s2sc: bad argument"); return E_ARG; }
  const int Fo = (Fi - 1) / 2 + 1, To = (Ti - 1) / 2 + 1;
  const int FPi = Fi + 2, TPi = Ti + 2, FPo = Fo + 2, TPo = To + 2;
  const size_t ni = (size_t)B * FPi * TPi * 32, no = (size_t)B * FPo * TPo * 64;
  std::vector<bf16_t> xb(ni, 0);
  for (int bb = 0; bb < B; ++bb)
    for (int f = 0; f < Fi; ++f)
      for (int t = 0; t < Ti; ++t)
        for (int c = 0; c < 32; ++c) xb[(((size_t)bb * FPi + f + 1) * TPi + t + 1) * 32 + c] = f32_to_bf16(x[(((size_t)bb * Fi + f) * Ti + t) * 32 + c]);
  std::vector<bf16_t> pw((size_t)9 * 64 * 32), ps((size_t)64 * 32);      // [o][ci][kh][kw] -> [tap][1][o][ci];  [o][ci] as it is
  for (int o = 0; o < 64; ++o)
    for (int ci = 0; ci < 32; ++ci) {
      for (int t = 0; t < 9; ++t) pw[((size_t)t * 64 + o) * 32 + ci] = f32_to_bf16(w[((size_t)o * 32 + ci) * 9 + t]);
      ps[(size_t)o * 32 + ci] = f32_to_bf16(wsc[(size_t)o * 32 + ci]);
    }
  Dev dx, dw, ds, db, dbs, dout, dsc;
  RVB_TRY(up_raw(dx, xb.data(), ni * 2)); RVB_TRY(up_raw(dw, pw.data(), pw.size() * 2)); RVB_TRY(up_raw(ds, ps.data(), ps.size() * 2));
  RVB_TRY(up_raw(db, b, 64 * 4)); RVB_TRY(up_raw(dbs, bsc, 64 * 4));
  RVB_TRY(dout.alloc(no * 2 + 256)); RVB_HIP_CHECK(hipMemset(dout.p, 0, no * 2 + 256));
  RVB_TRY(dsc.alloc(no * 2 + 256)); RVB_HIP_CHECK(hipMemset(dsc.p, 0, no * 2 + 256));
  if (!conv_s2sc_applicable(DT_BF16, 32, 64, 2, 9, 32, 64, 2, 1, Fi, Ti, Fo, To)) { set_error("rvb_test_conv_s2sc: switched off (RVD_CONV_S2SC=0)"); return E_STATE; }
  ConvS2Args a{};
  a.in = dx.p; a.w = dw.p; a.bias = (const float*)db.p; a.wsc = ds.p; a.bsc = (const float*)dbs.p; a.out = dout.p; a.sc = dsc.p;
  a.B = B; a.Fi = Fi; a.Ti = Ti; a.Fo = Fo; a.To = To;
  RVB_TRY(conv_s2sc(nullptr, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  std::vector<bf16_t> ob(no), sb(no);
  RVB_HIP_CHECK(hipMemcpy(ob.data(), dout.p, no * 2, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(sb.data(), dsc.p, no * 2, hipMemcpyDeviceToHost));
  for (int bb = 0; bb < B; ++bb)
    for (int f = 0; f < FPo; ++f)
      for (int t = 0; t < TPo; ++t)
        for (int c = 0; c < 64; ++c) {
          const size_t at = (((size_t)bb * FPo + f) * TPo + t) * 64 + c;
          if (f == 0 || f == FPo - 1 || t == 0 || t == TPo - 1) {
            // the zero border of both output planes must be untouched (the next convolution relies on it)
            if (ob[at] != 0 || sb[at] != 0) { set_error("rvb_test_conv_s2sc: the kernel wrote into the zero border"); return E_STATE; }
          } else {
            const size_t o = (((size_t)bb * Fo + f - 1) * To + t - 1) * 64 + c;
            out[o] = bf16_to_f32(ob[at]); sc[o] = bf16_to_f32(sb[at]);
          }
        }
  return OK;
}

int rvb_test_glu_dwconv(int dtype, const float* G, const float* pw1_bias, const float* dw_w, const float* dw_b,
                        const int32_t* lens, float* out, int B, int T, int d, int K, int causal, const float* hist,
                        int hist_rows) {
  RVB_TRY(need_gpu());
  Dev dG, dpb, dw, db, dl, dout, dh;
  const bool gated = (causal & 4) != 0;          // bit 2 of `causal`: G is [B][T][d], gated already (GluDwArgs::gated)
  RVB_TRY(up_T(dG, dtype, G, (size_t)B * T * (gated ? 1 : 2) * d));
  RVB_TRY(up_raw(dpb, pw1_bias, (size_t)2 * d * 4));
  std::vector<float> wt((size_t)d * K);            // the caller passes depthwise_conv.weight as the reference stores it, [d][K]
  for (int c = 0; c < d; ++c)
    for (int k = 0; k < K; ++k) wt[(size_t)k * d + c] = dw_w[(size_t)c * K + k];
  RVB_TRY(up_raw(dw, wt.data(), (size_t)d * K * 4));
  RVB_TRY(up_raw(db, dw_b, (size_t)d * 4));
  RVB_TRY(up_raw(dl, lens, (size_t)B * 4));
  const bool o16 = (causal & 2) != 0;            // bit 1 of `causal`: bf16 output (bf16 engine)
  causal &= 1;
  RVB_TRY(dout.alloc((size_t)B * T * d * 4));
  RVB_HIP_CHECK(hipMemset(dout.p, 0xff, (size_t)B * T * d * 4));      // NaN in fp32 and in bf16: a frame the kernel skipped shows
  GluDwArgs a;
  a.out_bf16 = o16 ? 1 : 0;
  a.gated = gated ? 1 : 0;
  a.G = dG.p; a.pw1_bias = (const float*)dpb.p; a.dw_w = (const float*)dw.p; a.dw_b = (const float*)db.p;
  a.lens = (const int*)dl.p; a.out = (float*)dout.p; a.B = B; a.T = T; a.d = d; a.K = K;
  a.causal = causal;
  if (hist && hist_rows > 0) {      // [K-1][2d], the last hist_rows rows are real frames
    RVB_TRY(up_T(dh, dtype, hist, (size_t)(K - 1) * 2 * d));
    a.hist = dh.p; a.hist_rows = hist_rows;
  }
  RVB_TRY(glu_dwconv(nullptr, dtype, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (o16) return down_T(dout, DT_BF16, false, out, (size_t)B * T * d);
  RVB_HIP_CHECK(hipMemcpy(out, dout.p, (size_t)B * T * d * 4, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_dwconv_ln(const float* G, const float* pw1_bias, const float* dw_w, const float* dw_b, const int32_t* lens,
                       const float* gamma, const float* beta, float eps, float* xn, float* xn_two, float* dconv_two, int B, int T,
                       int d, int K, int grid) {
  if (!G || !pw1_bias || !dw_w || !dw_b || !lens || !gamma || !beta || !xn || B < 1 || T < 1 || d < 1 || K < 1 || grid < 0) {
    set_error("rvb_test_dwconv_ln: null argument or a size < 1"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  const size_t n = (size_t)B * T * d;
  Dev dG, dpb, dw, db, dl, dg, dbe, dout, dconv, dout2;
  RVB_TRY(up_T(dG, DT_BF16, G, n));
  RVB_TRY(up_raw(dpb, pw1_bias, (size_t)2 * d * 4));
  std::vector<float> wt((size_t)d * K);            // tap-major on the device, as the engine keeps it
  for (int c = 0; c < d; ++c)
    for (int k = 0; k < K; ++k) wt[(size_t)k * d + c] = dw_w[(size_t)c * K + k];
  RVB_TRY(up_raw(dw, wt.data(), (size_t)d * K * 4));
  RVB_TRY(up_raw(db, dw_b, (size_t)d * 4));
  RVB_TRY(up_raw(dl, lens, (size_t)B * 4));
  RVB_TRY(up_raw(dg, gamma, (size_t)d * 4));
  RVB_TRY(up_raw(dbe, beta, (size_t)d * 4));
  RVB_TRY(dout.alloc(n * 2));
  RVB_HIP_CHECK(hipMemset(dout.p, 0xff, n * 2));
  DwLnArgs a;
  a.G = dG.p; a.pw1_bias = (const float*)dpb.p; a.dw_w = (const float*)dw.p; a.dw_b = (const float*)db.p; a.lens = (const int*)dl.p;
  a.gamma = (const float*)dg.p; a.beta = (const float*)dbe.p; a.eps = eps; a.out = dout.p; a.B = B; a.T = T; a.d = d; a.K = K; a.grid = grid;
  RVB_TRY(dwconv_ln(nullptr, DT_BF16, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_TRY(down_T(dout, DT_BF16, false, xn, n));
  if (!xn_two && !dconv_two) return OK;
  RVB_TRY(dconv.alloc(n * 2));
  RVB_HIP_CHECK(hipMemset(dconv.p, 0xff, n * 2));
  RVB_TRY(dout2.alloc(n * 2));
  RVB_HIP_CHECK(hipMemset(dout2.p, 0xff, n * 2));
  GluDwArgs g;
  g.G = dG.p; g.pw1_bias = a.pw1_bias; g.dw_w = a.dw_w; g.dw_b = a.dw_b; g.lens = a.lens; g.out = (float*)dconv.p;
  g.B = B; g.T = T; g.d = d; g.K = K; g.out_bf16 = 1; g.gated = 1;
  RVB_TRY(glu_dwconv(nullptr, DT_BF16, g));
  NormArgs nn;
  nn.x = (const float*)dconv.p; nn.x_bf16 = 1; nn.gamma = a.gamma; nn.beta = a.beta; nn.eps = eps; nn.mode = NORM_LN; nn.silu = 1;
  nn.add = nullptr; nn.out = dout2.p; nn.out_f32 = 0; nn.M = B * T; nn.d = d;
  RVB_TRY(rownorm(nullptr, DT_BF16, nn));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (dconv_two) RVB_TRY(down_T(dconv, DT_BF16, false, dconv_two, n));
  if (xn_two) RVB_TRY(down_T(dout2, DT_BF16, false, xn_two, n));
  return OK;
}

int rvb_test_attention(int dtype, const float* q, const float* k, const float* v, const float* p, const float* bias_u,
                       const float* bias_v, float* out, int q_rows, int kv_rows, int p_rows, int heads, int dk,
                       const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start, const int32_t* kv_len,
                       int nseq, int causal) {
  RVB_TRY(need_gpu());
  const int d = heads * dk;
  Dev dq, dkk, dv, dp, du, dvv, dout, qs, ql, ks, kl;
  RVB_TRY(up_T(dq, dtype, q, (size_t)q_rows * d));
  // bit 2 of `causal` (with bit 1, bf16): the keys go up PREFOLDED, K' = k + p[position of the key in its sequence] summed in fp32 and
  // rounded once -- what the qkv GEMM's epilogue writes in the engine (GemmArgs::rowadd); the kernel then runs with k_prefolded
  const bool prefolded = (causal & 6) == 6 && p && dtype == DT_BF16;
  if (prefolded) {
    std::vector<float> kp(k, k + (size_t)kv_rows * d);
    for (int i = 0; i < nseq; ++i)
      for (int j = 0; j < kv_len[i] && j < p_rows; ++j)
        for (int c = 0; c < d; ++c) kp[(size_t)(kv_start[i] + j) * d + c] += p[(size_t)j * d + c];
    RVB_TRY(up_T(dkk, dtype, kp.data(), (size_t)kv_rows * d));
  } else {
    RVB_TRY(up_T(dkk, dtype, k, (size_t)kv_rows * d));
  }
  RVB_TRY(up_T(dv, dtype, v, (size_t)kv_rows * d));
  RVB_TRY(up_T(dp, dtype, p, (size_t)p_rows * d));
  RVB_TRY(up_raw(du, bias_u, (size_t)d * 4));
  RVB_TRY(up_raw(dvv, bias_v, (size_t)d * 4));
  RVB_TRY(up_raw(qs, q_start, (size_t)nseq * 4));
  RVB_TRY(up_raw(ql, q_len, (size_t)nseq * 4));
  RVB_TRY(up_raw(ks, kv_start, (size_t)nseq * 4));
  RVB_TRY(up_raw(kl, kv_len, (size_t)nseq * 4));
  RVB_TRY(dout.alloc((size_t)q_rows * d * dt_size(dtype)));
  RVB_HIP_CHECK(hipMemset(dout.p, 0, (size_t)q_rows * d * dt_size(dtype)));
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = dq.p; a.k = dkk.p; a.v = dv.p; a.p = dp.p;
  a.q_stride = a.k_stride = a.v_stride = a.p_stride = a.o_stride = d;
  a.bias_u = (const float*)du.p; a.bias_v = (const float*)dvv.p; a.out = dout.p;
  a.q_start = (const int*)qs.p; a.q_len = (const int*)ql.p; a.kv_start = (const int*)ks.p; a.kv_len = (const int*)kl.p;
  // `causal`: bit 0 = causal mask; bit 1 = folded positional term; bit 2 = ... with prefolded keys (see above); bits 8..19 = streaming chunk size (0 = off); bits 20..31 = left chunks + 1 (0 = all)
  a.nseq = nseq; a.heads = heads; a.dk = dk; a.causal = causal & 1; a.sqrt_dk = sqrtf((float)dk);
  a.chunk = (causal >> 8) & 0xfff; a.left = ((causal >> 20) & 0xfff) - 1;
  int mq = 0;
  for (int i = 0; i < nseq; ++i) mq = q_len[i] > mq ? q_len[i] : mq;
  a.max_q = mq;
  // bit 1 of `causal`: the bf16 encoder form with the positional term folded into per-key constants (as the engine runs it)
  Dev dc;
  if ((causal & 2) && p && dtype == DT_BF16) {
    RVB_TRY(dc.alloc((size_t)heads * p_rows * 4));
    RVB_TRY(attention_pos_bias(nullptr, dp.p, p_rows, d, (const float*)du.p, (const float*)dvv.p, heads, dk, 1.44269504f / sqrtf((float)dk),
                             (float*)dc.p));
    a.pos_bias = (const float*)dc.p; a.pos_bias_stride = p_rows;
    int mk = 0;
    for (int i = 0; i < nseq; ++i) mk = kv_len[i] > mk ? kv_len[i] : mk;
    a.fold_kv_cap = (mk + 63) / 64 * 64;
    a.k_prefolded = prefolded ? 1 : 0;
  }
  attention_lab_switches(a);      // RVB_ATTN_* of the lab build, as the engine passes them
  RVB_TRY(attention(nullptr, dtype, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, false, out, (size_t)q_rows * d);
}

// ragged / shared-prefix form of the decoder self attention: keys through an index list, queries that start at
// position q_pos0 of their key sequence, 16-query blocks from a work list
int rvb_test_attention_trie(int dtype, const float* q, const float* k, const float* v, float* out, int rows, int heads, int dk,
                            const int32_t* q_start, const int32_t* q_len, const int32_t* q_pos0, const int32_t* kv_start,
                            const int32_t* kv_len, const int32_t* kv_index, int n_index, int nseq, int q_block) {
  RVB_TRY(need_gpu());
  const int d = heads * dk;
  Dev dq, dkk, dv, dout, qs, ql, qp, ks, kl, ki, wk;
  RVB_TRY(up_T(dq, dtype, q, (size_t)rows * d));
  RVB_TRY(up_T(dkk, dtype, k, (size_t)rows * d));
  RVB_TRY(up_T(dv, dtype, v, (size_t)rows * d));
  RVB_TRY(up_raw(qs, q_start, (size_t)nseq * 4)); RVB_TRY(up_raw(ql, q_len, (size_t)nseq * 4)); RVB_TRY(up_raw(qp, q_pos0, (size_t)nseq * 4));
  RVB_TRY(up_raw(ks, kv_start, (size_t)nseq * 4)); RVB_TRY(up_raw(kl, kv_len, (size_t)nseq * 4));
  RVB_TRY(up_raw(ki, kv_index, (size_t)n_index * 4));
  RVB_TRY(dout.alloc((size_t)rows * d * dt_size(dtype)));
  RVB_HIP_CHECK(hipMemset(dout.p, 0, (size_t)rows * d * dt_size(dtype)));
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = dq.p; a.k = dkk.p; a.v = dv.p;
  a.q_stride = a.k_stride = a.v_stride = a.o_stride = d; a.out = dout.p;
  a.q_start = (const int*)qs.p; a.q_len = (const int*)ql.p; a.q_pos0 = (const int*)qp.p;
  a.kv_start = (const int*)ks.p; a.kv_len = (const int*)kl.p; a.kv_index = (const int*)ki.p;
  a.nseq = nseq; a.heads = heads; a.dk = dk; a.causal = 1; a.sqrt_dk = sqrtf((float)dk); a.q_block = q_block;
  int mq = 0;
  std::vector<int32_t> work;
  const int qb = q_block == 16 ? 16 : 128;
  for (int i = 0; i < nseq; ++i) {
    mq = q_len[i] > mq ? q_len[i] : mq;
    for (int q0 = 0; q0 < q_len[i]; q0 += qb) { work.push_back(i); work.push_back(q0); }
  }
  a.max_q = mq;
  if (q_block == 16) {      // the work-list launch (what the engine uses); q_block 0: the plain (x, z) grid
    RVB_TRY(up_raw(wk, work.data(), work.size() * 4));
    a.work = (const int*)wk.p; a.n_work = (int)work.size() / 2;
  }
  attention_lab_switches(a);      // RVB_ATTN_* of the lab build, as the engine passes them
  RVB_TRY(attention(nullptr, dtype, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, false, out, (size_t)rows * d);
}

// attention() as the engine calls it: strided / fused operand buffers, positional rows from an offset, fold, index list, work list,
// block size, masks, lab switches; reports the instantiation launch_attn chose.  All checks come before any device work.
static int attn_ex_check(const rvb_test_attn_args& t) {
  auto bad = [](const char* m) { set_error(std::string("rvb_test_attention_ex: ") + m); return E_ARG; };
  if (t.dtype != DT_F32 && t.dtype != DT_BF16) return bad("dtype");
  if (t.heads <= 0 || t.dk <= 0 || t.nseq <= 0 || t.heads > 64 || t.dk > 4096) return bad("heads / dk / nseq");
  if (!t.q || !t.k || !t.v || !t.out || !t.q_start || !t.q_len || !t.kv_start || !t.kv_len) return bad("null operand");
  const int d = t.heads * t.dk, ve = t.dtype == DT_BF16 ? 8 : 4;
  auto cols = [&](int rows, int stride, int col, int align) { return rows >= 0 && stride > 0 && col >= 0 && col % align == 0 && (int64_t)col + d <= stride; };
  if (!cols(t.q_rows, t.q_stride, t.q_col, ve) || !cols(t.k_rows, t.k_stride, t.k_col, ve) || !cols(t.v_rows, t.v_stride, t.v_col, ve))
    return bad("q / k / v: head columns outside the row, or not on a 16-byte boundary");
  if (!cols(t.o_rows, t.o_stride, t.o_col, 4)) return bad("out: head columns outside the row, or not on a 4-element boundary");
  // buffers named by one host pointer are one device buffer: they must agree on its shape
  if ((t.q == t.k && (t.q_rows != t.k_rows || t.q_stride != t.k_stride)) || (t.q == t.v && (t.q_rows != t.v_rows || t.q_stride != t.v_stride)) ||
      (t.k == t.v && (t.k_rows != t.v_rows || t.k_stride != t.v_stride)))
    return bad("operands that share a buffer disagree on its rows / stride");
  if ((t.bias_u == nullptr) != (t.bias_v == nullptr)) return bad("bias_u / bias_v come together");
  if (t.n_index < 0 || (t.kv_index == nullptr) != (t.n_index == 0)) return bad("kv_index / n_index");
  if (t.n_work < 0 || (t.work == nullptr) != (t.n_work == 0)) return bad("work / n_work");
  if (t.chunk < 0 || t.max_q < 0 || t.fold_kv_cap < 0 || t.p_off < 0) return bad("negative chunk / max_q / fold_kv_cap / p_off");
  const int kv_rows = t.k_rows < t.v_rows ? t.k_rows : t.v_rows;
  int max_kv = 0;
  for (int i = 0; i < t.nseq; ++i) {
    if (t.q_start[i] < 0 || t.q_len[i] < 0 || (int64_t)t.q_start[i] + t.q_len[i] > t.q_rows || (int64_t)t.q_start[i] + t.q_len[i] > t.o_rows)
      return bad("a sequence's queries lie outside q / out");
    if (t.kv_start[i] < 0 || t.kv_len[i] < 0 || (int64_t)t.kv_start[i] + t.kv_len[i] > (t.kv_index ? t.n_index : kv_rows))
      return bad("a sequence's keys lie outside k / v (or the index list)");
    if (t.q_pos0 && t.q_pos0[i] < 0) return bad("negative q_pos0");
    max_kv = t.kv_len[i] > max_kv ? t.kv_len[i] : max_kv;
  }
  for (int i = 0; i < t.n_index; ++i)
    if (t.kv_index[i] < 0 || t.kv_index[i] >= kv_rows) return bad("kv_index entry outside k / v");
  for (int i = 0; i < t.n_work; ++i)
    if (t.work[2 * i] < 0 || t.work[2 * i] >= t.nseq || t.work[2 * i + 1] < 0) return bad("work list entry");
  if (t.p) {
    if (t.p_rows <= 0 || t.p_stride <= 0 || t.p_col < 0 || t.p_col % ve || (int64_t)t.p_col + d > t.p_stride || t.p_off >= t.p_rows)
      return bad("p: head columns outside the row, not on a 16-byte boundary, or p_off past the last row");
    if (!t.bias_u) return bad("positional keys need bias_u / bias_v");
    // prefolded keys: the kernel reads no positional row, only the table (clamped at its last entry)
    if (!(t.fold && t.k_prefolded) && (int64_t)t.p_off + max_kv > t.p_rows) return bad("positional rows p_off .. p_off + kv_len lie outside p");
  }
  if (t.fold && (!t.p || t.dtype != DT_BF16)) return bad("fold needs bf16 positional keys");
  if (t.fold && t.fold_kv_cap < max_kv) return bad("fold_kv_cap must cover every sequence's kv_len");
  if (t.k_prefolded && !t.fold) return bad("k_prefolded without fold");
  return OK;
}

int rvb_test_attention_ex(rvb_test_attn_args* tp) {
  if (!tp) { set_error("rvb_test_attention_ex: null"); return E_ARG; }
  rvb_test_attn_args& t = *tp;
  for (int i = 0; i < 8; ++i) t.ran[i] = 0;
  RVB_TRY(attn_ex_check(t));
  RVB_TRY(need_gpu());
  const int dtype = t.dtype, d = t.heads * t.dk;
  const size_t es = dt_size(dtype);
  Dev dq, dkk, dv, dp, du, dvv, dout, dc, qs, ql, ks, kl, qp, ki, wk;
  RVB_TRY(up_T(dq, dtype, t.q, (size_t)t.q_rows * t.q_stride));
  if (t.k != t.q) RVB_TRY(up_T(dkk, dtype, t.k, (size_t)t.k_rows * t.k_stride));
  if (t.v != t.q && t.v != t.k) RVB_TRY(up_T(dv, dtype, t.v, (size_t)t.v_rows * t.v_stride));
  const char* bq = (const char*)dq.p;
  const char* bk = t.k == t.q ? bq : (const char*)dkk.p;
  const char* bv = t.v == t.q ? bq : t.v == t.k ? bk : (const char*)dv.p;
  RVB_TRY(up_T(dout, dtype, t.out, (size_t)t.o_rows * t.o_stride));
  if (t.p) RVB_TRY(up_T(dp, dtype, t.p, (size_t)t.p_rows * t.p_stride));
  RVB_TRY(up_raw(du, t.bias_u, (size_t)d * 4));
  RVB_TRY(up_raw(dvv, t.bias_v, (size_t)d * 4));
  RVB_TRY(up_raw(qs, t.q_start, (size_t)t.nseq * 4)); RVB_TRY(up_raw(ql, t.q_len, (size_t)t.nseq * 4));
  RVB_TRY(up_raw(ks, t.kv_start, (size_t)t.nseq * 4)); RVB_TRY(up_raw(kl, t.kv_len, (size_t)t.nseq * 4));
  RVB_TRY(up_raw(qp, t.q_pos0, (size_t)t.nseq * 4));
  RVB_TRY(up_raw(ki, t.kv_index, (size_t)t.n_index * 4));
  RVB_TRY(up_raw(wk, t.work, (size_t)t.n_work * 8));
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = bq + (size_t)t.q_col * es; a.k = bk + (size_t)t.k_col * es; a.v = bv + (size_t)t.v_col * es;
  a.out = (char*)dout.p + (size_t)t.o_col * es;
  a.q_stride = t.q_stride; a.k_stride = t.k_stride; a.v_stride = t.v_stride; a.o_stride = t.o_stride;
  if (t.p) { a.p = (const char*)dp.p + ((size_t)t.p_off * t.p_stride + t.p_col) * es; a.p_stride = t.p_stride; }
  a.bias_u = (const float*)du.p; a.bias_v = (const float*)dvv.p;
  a.q_start = (const int*)qs.p; a.q_len = (const int*)ql.p; a.kv_start = (const int*)ks.p; a.kv_len = (const int*)kl.p;
  a.q_pos0 = (const int*)qp.p; a.kv_index = (const int*)ki.p; a.work = (const int*)wk.p; a.n_work = t.n_work;
  a.nseq = t.nseq; a.heads = t.heads; a.dk = t.dk; a.causal = t.causal ? 1 : 0; a.chunk = t.chunk; a.left = t.left;
  a.sqrt_dk = sqrtf((float)t.dk); a.q_block = t.q_block; a.plain_order = t.plain_order ? 1 : 0; a.lab = t.lab;
  a.max_q = t.max_q;
  if (a.max_q == 0)
    for (int i = 0; i < t.nseq; ++i) a.max_q = t.q_len[i] > a.max_q ? t.q_len[i] : a.max_q;
  if (t.fold) {
    const int rows = t.p_rows - t.p_off;
    RVB_TRY(dc.alloc((size_t)t.heads * rows * 4));
    RVB_TRY(attention_pos_bias(nullptr, a.p, rows, t.p_stride, a.bias_u, a.bias_v, t.heads, t.dk, 1.44269504f / sqrtf((float)t.dk), (float*)dc.p));
    a.pos_bias = (const float*)dc.p; a.pos_bias_stride = rows; a.fold_kv_cap = t.fold_kv_cap; a.k_prefolded = t.k_prefolded ? 1 : 0;
  }
  (void)attention_last_form(true);
  const int rc = attention(nullptr, dtype, a);
  const AttnForm f = attention_last_form(true);
  const int ran[8] = {f.elem_size, f.dkp, f.has_pos, f.nw, f.fold, f.padk, f.occ, f.mf};
  for (int i = 0; i < 8; ++i) t.ran[i] = ran[i];
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_TRY(down_T(dout, dtype, false, t.out, (size_t)t.o_rows * t.o_stride));      // also after a refusal: the sentinel must be intact
  return rc;
}

int rvb_test_attention_pos_bias(const float* p, int p_rows, int p_stride, int p_col, int p_off, const float* bias_u, const float* bias_v,
                                int heads, int dk, float scale, float* out) {
  if (!p || !bias_u || !bias_v || !out || heads <= 0 || dk <= 0 || p_rows <= 0 || p_stride <= 0 || p_col < 0 || p_off < 0 || p_off >= p_rows ||
      (int64_t)p_col + (int64_t)heads * dk > p_stride) {
    set_error("rvb_test_attention_pos_bias: head columns outside the row, or p_off past the last row");
    return E_ARG;
  }
  RVB_TRY(need_gpu());
  Dev dp, du, dvv, dc;
  const int rows = p_rows - p_off;
  RVB_TRY(up_T(dp, DT_BF16, p, (size_t)p_rows * p_stride));
  RVB_TRY(up_raw(du, bias_u, (size_t)heads * dk * 4));
  RVB_TRY(up_raw(dvv, bias_v, (size_t)heads * dk * 4));
  RVB_TRY(dc.alloc((size_t)heads * rows * 4));
  RVB_TRY(attention_pos_bias(nullptr, (const bf16_t*)dp.p + (size_t)p_off * p_stride + p_col, rows, p_stride, (const float*)du.p, (const float*)dvv.p,
                           heads, dk, scale, (float*)dc.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(out, dc.p, (size_t)heads * rows * 4, hipMemcpyDeviceToHost));
  return OK;
}

// the three row_lse_kernel entry points on host logits [M][ld] (test_api.h): outputs start as all-ones bytes on the device
static int rowlse_args(const char* who, const float* logits, int M, int V, int ld) {
  const std::string me(who);
  if (!logits || M < 1) { set_error(me + ": null logits or fewer than one row"); return E_ARG; }
  if (V < 1) { set_error(me + ": V < 1"); return E_ARG; }
  if (ld < V) { set_error(me + ": ld < V"); return E_ARG; }
  return OK;
}

int rvb_test_logsoftmax_topk_ex(const float* logits, int M, int V, int ld, int k, float blank_penalty, int blank_id,
                                float* topk_val, int32_t* topk_idx, float* logp) {
  RVB_TRY(rowlse_args("rvb_test_logsoftmax_topk_ex", logits, M, V, ld));
  if (!topk_val || !topk_idx) { set_error("rvb_test_logsoftmax_topk_ex: null output"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dl, dv, di, dp;
  const size_t nk = (size_t)M * (size_t)std::max(k, 1) * 4, nlp = (size_t)M * V * 4;    // a k the launcher is going to refuse still gets buffers
  RVB_TRY(up_raw(dl, logits, (size_t)M * ld * 4));
  RVB_TRY(dv.alloc(nk)); RVB_HIP_CHECK(hipMemset(dv.p, 0xff, nk));
  RVB_TRY(di.alloc(nk)); RVB_HIP_CHECK(hipMemset(di.p, 0xff, nk));
  if (logp) { RVB_TRY(dp.alloc(nlp)); RVB_HIP_CHECK(hipMemset(dp.p, 0xff, nlp)); }
  RVB_TRY(logsoftmax_topk(nullptr, (const float*)dl.p, M, V, ld, k, blank_penalty, blank_id, (float*)dv.p, (int*)di.p,
                        (float*)dp.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(topk_val, dv.p, nk, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(topk_idx, di.p, nk, hipMemcpyDeviceToHost));
  if (logp) RVB_HIP_CHECK(hipMemcpy(logp, dp.p, nlp, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_logsoftmax_topk(const float* logits, int M, int V, int k, float blank_penalty, int blank_id,
                             float* topk_val, int32_t* topk_idx, float* logp) {
  return rvb_test_logsoftmax_topk_ex(logits, M, V, V, k, blank_penalty, blank_id, topk_val, topk_idx, logp);
}

static int ctc_viterbi_lab(const char* who, bool wild, const float* lp, int T, int V, const float* w, float bias, const int32_t* tokens,
                           int L, int blank, int slab_rows, int32_t* labels_out, float* score_out) {
  const std::string me(who);
  if (!lp || !tokens || !labels_out || !score_out || (wild && !w)) { set_error(me + ": null argument"); return E_ARG; }
  if (T < 1 || slab_rows < 1) { set_error(me + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  if (wild && !(std::isfinite(bias) && bias <= 0.f)) { set_error(me + ": wildcard bias must be finite and <= 0"); return E_ARG; }
  CtcAligner al;
  std::vector<std::vector<int32_t>> rows;
  lab_rows(&T, 1, &rows);
  RVB_TRY(al.plan(who, tokens, &L, 1, rows, V, blank, wild));
  std::vector<int32_t> states;
  float score = 0.f;
  RVB_TRY(lab_align(al, lp, wild ? w : nullptr, T, V, slab_rows, bias, &states, &score));
  *score_out = score;
  for (int t = 0; t < T; ++t) labels_out[t] = (states[t] & 1) ? tokens[states[t] >> 1] : blank;
  return OK;
}

int rvb_test_ctc_viterbi(const float* lp, int T, int V, const int32_t* tokens, int L, int blank, int slab_rows, int32_t* labels_out,
                         float* score_out) {
  return ctc_viterbi_lab("rvb_test_ctc_viterbi", false, lp, T, V, nullptr, 0.f, tokens, L, blank, slab_rows, labels_out, score_out);
}

int rvb_test_ctc_viterbi_wild(const float* lp, int T, int V, const float* w, float bias, const int32_t* tokens, int L, int blank,
                              int slab_rows, int32_t* labels_out, float* score_out) {
  return ctc_viterbi_lab("rvb_test_ctc_viterbi_wild", true, lp, T, V, w, bias, tokens, L, blank, slab_rows, labels_out, score_out);
}

int rvb_test_ctc_viterbi_window(const float* lp, int T, int V, const float* w, float bias, const int32_t* tokens, int L, int blank,
                                int slab_rows, int window_states, int32_t* labels_out, float* score_out, int32_t* lo_out,
                                int32_t* min_margin_out) {
  const char* who = "rvb_test_ctc_viterbi_window";
  const std::string me(who);
  if (!lp || !tokens || !labels_out || !score_out || !lo_out || !min_margin_out) { set_error(me + ": null argument"); return E_ARG; }
  if (T < 1 || slab_rows < 1) { set_error(me + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  CtcWindowAligner al;
  RVB_TRY(al.plan(who, tokens, L, T, window_states, V, blank, w != nullptr, bias));
  al.has_wild = w != nullptr;                      // w selects the WILD kernels, whether or not a token is a wildcard
  RVB_TRY(need_gpu());
  Dev dlp, dw;
  std::vector<int32_t> rows((size_t)T), states((size_t)T), los((size_t)T);
  for (int t = 0; t < T; ++t) rows[t] = t;
  float score = 0.f;
  int32_t margin = 0;
  int r = up_raw(dlp, lp, (size_t)T * V * 4);
  if (r == OK) r = up_raw(dw, w, (size_t)T * 4);
  if (r == OK) r = al.begin(nullptr);
  if (r == OK) r = al.batch(nullptr, rows);
  r = feed_slabs(r, T, slab_rows, false, [&](int r0, int n) {
    return al.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n, w ? (const float*)dw.p + r0 : nullptr);
  });
  if (r == OK) r = al.finish(nullptr, states.data(), &score, &margin, los.data());
  if (r != OK) (void)hipDeviceSynchronize();
  al.release();
  RVB_TRY(r);
  *score_out = score;
  *min_margin_out = margin;
  for (int t = 0; t < T; ++t) {
    labels_out[t] = (states[t] & 1) ? tokens[states[t] >> 1] : blank;
    lo_out[t] = los[t];
  }
  return OK;
}

int rvb_test_ctc_window_next_lo(int S, int T, int W, int f0, int f1, int lo_prev, int best_prev) {
  return ctc_window_next_lo(S, T, W, f0, f1, lo_prev, best_prev);
}

int rvb_test_ctc_viterbi_graph(const float* lp, const int32_t* T, int n_seq, int V, const float* w, float bias, const int32_t* node_tokens,
                               const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final, int blank,
                               int slab_rows, int32_t* labels_out, int32_t* frame_node_out, float* score_out) {
  const std::string me("rvb_test_ctc_viterbi_graph");
  if (!lp || !T || !node_tokens || !n_nodes || !pred_off || !preds || !is_final || !labels_out || !frame_node_out || !score_out) {
    set_error(me + ": null argument");
    return E_ARG;
  }
  if (n_seq < 1 || slab_rows < 1) { set_error(me + ": need n_seq >= 1 and slab_rows >= 1"); return E_ARG; }
  if (!(std::isfinite(bias) && bias <= 0.f)) { set_error(me + ": wildcard_bias must be finite and <= 0"); return E_ARG; }
  CtcGraphAligner al;
  for (int i = 0; i < n_seq; ++i)
    if (T[i] < 1) { set_error(me + ": sequence " + std::to_string(i) + ": need T >= 1"); return E_ARG; }
  std::vector<std::vector<int32_t>> rows;
  const int64_t M = lab_rows(T, n_seq, &rows);
  RVB_TRY(al.plan(me.c_str(), node_tokens, n_nodes, pred_off, preds, is_final, n_seq, rows, V, blank));
  if (al.has_wild && !w) { set_error(me + ": a graph with wildcards needs w"); return E_ARG; }
  std::vector<int32_t> states;
  std::vector<float> score(n_seq);
  RVB_TRY(lab_align(al, lp, w, M, V, slab_rows, bias, &states, score.data()));
  memcpy(score_out, score.data(), (size_t)n_seq * 4);
  for (int i = 0; i < n_seq; ++i) {
    const GraphSeq& q = al.seq[i];
    for (int t = 0; t < q.T; ++t) {
      const int st = states[q.frame_off + t], node = (st >> 1) - 1;
      frame_node_out[q.frame_off + t] = (st & 1) ? node : -1;
      labels_out[q.frame_off + t] = (st & 1) ? node_tokens[q.node_off + node] : blank;
    }
  }
  return OK;
}

int rvb_test_ctc_graph_window(const float* lp, int T, int V, const float* w, float bias, const int32_t* node_tokens, int n_nodes,
                              const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final, int blank, int slab_rows, int window_nodes,
                              const int32_t* lo_force, int32_t* labels_out, int32_t* frame_node_out, float* score_out, int32_t* lo_out,
                              int32_t* min_margin_out, int32_t* launches_out) {
  const char* who = "rvb_test_ctc_graph_window";
  const std::string me(who);
  if (!lp || !node_tokens || !pred_off || !preds || !is_final || !labels_out || !frame_node_out || !score_out || !lo_out || !min_margin_out ||
      !launches_out) { set_error(me + ": null argument"); return E_ARG; }
  if (T < 1 || slab_rows < 1) { set_error(me + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  CtcGraphWindowAligner al;
  RVB_TRY(al.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, T, window_nodes, V, blank, bias));
  if (al.has_wild && !w) { set_error(me + ": a graph with wildcards needs w"); return E_ARG; }
  if (lo_force) {
    const int n_launch = (T + slab_rows - 1) / slab_rows, top = std::max(0, (al.N + 63) / 64 * 64 - al.W);
    for (int i = 0; i < n_launch; ++i) {
      const int v = lo_force[i];
      if (v % 64 != 0 || v < 0 || v > top || (i == 0 ? v != 0 : v < lo_force[i - 1])) {
        set_error(me + ": lo_force[" + std::to_string(i) + "] = " + std::to_string(v) + " must be a multiple of 64 in [0, " +
                  std::to_string(top) + "], not below the entry before it, and 0 for launch 0");
        return E_ARG;
      }
    }
    al.lo_force = lo_force;
    al.n_force = n_launch;
  }
  RVB_TRY(need_gpu());
  Dev dlp, dw;
  std::vector<int32_t> rows((size_t)T), states((size_t)T), los((size_t)T);
  for (int t = 0; t < T; ++t) rows[t] = t;
  float score = 0.f;
  int32_t margin = 0;
  int r = up_raw(dlp, lp, (size_t)T * V * 4);
  if (r == OK) r = up_raw(dw, w, (size_t)T * 4);
  if (r == OK) r = al.begin(nullptr);
  if (r == OK) r = al.batch(nullptr, rows);
  r = feed_slabs(r, T, slab_rows, false, [&](int r0, int n) {
    return al.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n, w ? (const float*)dw.p + r0 : nullptr);
  });
  if (r == OK) r = al.finish(nullptr, states.data(), &score, &margin, los.data());
  if (r != OK) (void)hipDeviceSynchronize();
  const int launches = al.launches;
  al.release();
  RVB_TRY(r);                                      // nothing was written so far: a refusal leaves every output untouched
  *score_out = score;
  *min_margin_out = margin;
  *launches_out = launches;
  for (int t = 0; t < T; ++t) {
    const int st = states[t], node = (st >> 1) - 1;
    frame_node_out[t] = (st & 1) ? node : -1;
    labels_out[t] = (st & 1) ? node_tokens[node] : blank;
    lo_out[t] = los[t];
  }
  return OK;
}

int rvb_test_ctc_graph_window_next(const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                   const uint8_t* is_final, int T, int V, int window_nodes, int n_query, const int32_t* f0,
                                   const int32_t* fend, const int32_t* lo_prev, const int32_t* best_prev, int32_t* lo_out, int32_t* f1_out) {
  const char* who = "rvb_test_ctc_graph_window_next";
  const std::string me(who);
  if (!f0 || !fend || !lo_prev || !best_prev || !lo_out || !f1_out || n_query < 0) { set_error(me + ": null argument"); return E_ARG; }
  CtcGraphWindowAligner al;
  RVB_TRY(al.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, T, window_nodes, V, 0, 0.f));
  const int top = std::max(0, (al.N + 63) / 64 * 64 - al.W);
  for (int i = 0; i < n_query; ++i)
    if (f0[i] < 0 || f0[i] >= fend[i] || fend[i] > T || lo_prev[i] < 0 || lo_prev[i] > top || lo_prev[i] % 64 != 0 || best_prev[i] < -1 ||
        best_prev[i] >= al.N) {
      set_error(me + ": query " + std::to_string(i) + " is outside the lattice");
      return E_ARG;
    }
  for (int i = 0; i < n_query; ++i) {
    const CtcGraphWindowStep st = ctc_graph_window_next(al.tab, T, al.W, f0[i], fend[i], lo_prev[i], best_prev[i]);
    lo_out[i] = st.lo; f1_out[i] = st.f1;
  }
  return OK;
}

static int ctc_score_lab(const char* who, const float* lp, const int32_t* T, int V, const int32_t* tokens, const int32_t* L, int n_seq,
                         int blank, int slab_rows, double* loglik_out, float* occupancy, float* mean_frame, float* peak_post,
                         int32_t* peak_frame) {
  const std::string w(who);
  if (!lp || !T || !tokens || !L || !loglik_out || n_seq < 1) { set_error(w + ": null argument"); return E_ARG; }
  if (slab_rows < 1) { set_error(w + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  CtcScorer sc;
  for (int i = 0; i < n_seq; ++i)
    if (T[i] < 1) { set_error(w + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  std::vector<std::vector<int32_t>> rows;
  const int64_t M = lab_rows(T, n_seq, &rows);
  RVB_TRY(sc.plan(who, tokens, L, n_seq, rows, V, blank));
  RVB_TRY(need_gpu());
  const bool post = occupancy || mean_frame || peak_post || peak_frame;
  Dev dlp;
  int r = up_raw(dlp, lp, (size_t)M * V * 4);
  if (r == OK) r = sc.begin(nullptr, post);
  r = feed_slabs(r, M, slab_rows, false, [&](int r0, int n) { return sc.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n); });
  if (r == OK) r = sc.finish_forward(nullptr, loglik_out);
  if (r == OK && post) {
    r = feed_slabs(r, M, slab_rows, true, [&](int r0, int n) { return sc.advance_backward(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n); });
    if (r == OK) r = sc.finish_backward(nullptr, occupancy, mean_frame, peak_post, peak_frame);
  }
  if (r != OK) (void)hipDeviceSynchronize();
  sc.release();
  return r;
}

int rvb_test_ctc_score(const float* lp, int T, int V, const int32_t* tokens, int L, int blank, int slab_rows, double* loglik_out,
                       float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  return ctc_score_lab("rvb_test_ctc_score", lp, &T, V, tokens, &L, 1, blank, slab_rows, loglik_out, occupancy, mean_frame, peak_post,
                       peak_frame);
}

int rvb_test_ctc_score_batch(const float* lp, const int32_t* T, int V, const int32_t* tokens, const int32_t* L, int n_seq, int blank,
                             int slab_rows, double* loglik_out, float* occupancy, float* mean_frame, float* peak_post,
                             int32_t* peak_frame) {
  return ctc_score_lab("rvb_test_ctc_score_batch", lp, T, V, tokens, L, n_seq, blank, slab_rows, loglik_out, occupancy, mean_frame,
                       peak_post, peak_frame);
}

int rvb_test_ctc_score_window(const float* lp, int T, int V, const int32_t* tokens, int L, int blank, int slab_rows, int window_states,
                              const int32_t* lo_force, double* loglik_out, float* occupancy, float* mean_frame, float* peak_post,
                              int32_t* peak_frame, int32_t* lo_out, int32_t* best_out) {
  const char* who = "rvb_test_ctc_score_window";
  const std::string me(who);
  if (!lp || !tokens || !loglik_out || !lo_out) { set_error(me + ": null argument"); return E_ARG; }
  if (T < 1 || slab_rows < 1) { set_error(me + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  CtcWindowScorer sc;
  RVB_TRY(sc.plan(who, tokens, L, T, window_states, V, blank));
  const int n_launch = sc.launch_count(slab_rows);
  if (lo_force) {
    for (int i = 0; i < n_launch; ++i) {
      const int v = lo_force[i];
      if (v % 32 != 0 || v < 0 || v > sc.S_pad - sc.W || (i == 0 ? v != 0 : v < lo_force[i - 1])) {
        set_error(me + ": lo_force[" + std::to_string(i) + "] = " + std::to_string(v) + " must be a multiple of 32 in [0, " +
                  std::to_string(sc.S_pad - sc.W) + "], not below the entry before it, and 0 for launch 0");
        return E_ARG;
      }
    }
    sc.lo_force = lo_force;
    sc.n_force = n_launch;
  }
  const bool post = occupancy || mean_frame || peak_post || peak_frame;
  if (post) RVB_TRY(sc.rows_fit());
  RVB_TRY(need_gpu());
  Dev dlp;
  std::vector<int32_t> rows((size_t)T);
  for (int t = 0; t < T; ++t) rows[t] = t;
  double ll = 0.0;
  int r = up_raw(dlp, lp, (size_t)T * V * 4);
  if (r == OK) r = sc.begin(nullptr, post);
  if (r == OK) r = sc.batch(nullptr, rows);
  r = feed_slabs(r, T, slab_rows, false, [&](int r0, int n) { return sc.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n); });
  if (r == OK) r = sc.finish_forward(nullptr, &ll);
  std::vector<float> occ((size_t)L), mean((size_t)L), peak((size_t)L);
  std::vector<int32_t> pf((size_t)L);
  if (r == OK && post) {
    r = sc.batch_backward(nullptr, rows);
    r = feed_slabs(r, T, slab_rows, true, [&](int r0, int n) { return sc.advance_backward(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n); });
    if (r == OK) r = sc.finish_backward(nullptr, occ.data(), mean.data(), peak.data(), pf.data());
  }
  if (r != OK) (void)hipDeviceSynchronize();
  const std::vector<CtcWindowScorer::Launch> launches = sc.launches;
  sc.release();
  RVB_TRY(r);                                      // nothing was written so far: a refusal leaves every output untouched
  *loglik_out = ll;
  for (const auto& m : launches)
    for (int t = m.f0; t < m.f1; ++t) lo_out[t] = m.lo;
  if (best_out)
    for (size_t i = 0; i < launches.size(); ++i) best_out[i] = launches[i].best;
  if (occupancy) memcpy(occupancy, occ.data(), (size_t)L * 4);
  if (mean_frame) memcpy(mean_frame, mean.data(), (size_t)L * 4);
  if (peak_post) memcpy(peak_post, peak.data(), (size_t)L * 4);
  if (peak_frame) memcpy(peak_frame, pf.data(), (size_t)L * 4);
  return OK;
}

int rvb_test_ctc_score_graph(const float* lp, const int32_t* T, int n_seq, int V, const int32_t* node_tokens, const int32_t* n_nodes,
                             const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final, int blank, int slab_rows,
                             double* loglik_out, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame) {
  const char* who = "rvb_test_ctc_score_graph";
  const std::string w(who);
  if (!lp || !T || !node_tokens || !n_nodes || !pred_off || !preds || !is_final || !loglik_out) { set_error(w + ": null argument"); return E_ARG; }
  if (n_seq < 1 || slab_rows < 1) { set_error(w + ": need n_seq >= 1 and slab_rows >= 1"); return E_ARG; }
  for (int i = 0; i < n_seq; ++i)
    if (T[i] < 1) { set_error(w + ": sequence " + std::to_string(i) + ": need T >= 1"); return E_ARG; }
  CtcGraphScorer sc;
  std::vector<std::vector<int32_t>> rows;
  const int64_t M = lab_rows(T, n_seq, &rows);
  const bool post = visit || occupancy || mean_frame || peak_post || peak_frame;
  RVB_TRY(sc.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, n_seq, rows, V, blank, post));
  RVB_TRY(need_gpu());
  Dev dlp;
  std::vector<double> ll((size_t)n_seq);
  int r = up_raw(dlp, lp, (size_t)M * V * 4);
  if (r == OK) r = sc.begin(nullptr);
  r = feed_slabs(r, M, slab_rows, false, [&](int r0, int n) { return sc.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n); });
  if (r == OK) r = sc.finish_forward(nullptr, ll.data());
  if (r == OK && post) {
    r = feed_slabs(r, M, slab_rows, true, [&](int r0, int n) { return sc.advance_backward(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n); });
    if (r == OK) r = sc.finish_backward(nullptr, visit, occupancy, mean_frame, peak_post, peak_frame);
  }
  if (r == OK) memcpy(loglik_out, ll.data(), (size_t)n_seq * 8);
  if (r != OK) (void)hipDeviceSynchronize();
  sc.release();
  return r;
}

int rvb_test_ctc_score_graph_window(const float* lp, int T, int V, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off,
                                    const int32_t* preds, const uint8_t* is_final, int blank, int slab_rows, int window_nodes,
                                    const int32_t* lo_force, double* loglik_out, float* visit, float* occupancy, float* mean_frame,
                                    float* peak_post, int32_t* peak_frame, int32_t* lo_out, int32_t* best_out, int32_t* launches_out) {
  const char* who = "rvb_test_ctc_score_graph_window";
  const std::string me(who);
  if (!lp || !node_tokens || !pred_off || !preds || !is_final || !loglik_out || !lo_out) { set_error(me + ": null argument"); return E_ARG; }
  if (T < 1 || slab_rows < 1) { set_error(me + ": need T >= 1 and slab_rows >= 1"); return E_ARG; }
  const bool post = visit || occupancy || mean_frame || peak_post || peak_frame;
  CtcGraphWindowScorer sc;
  RVB_TRY(sc.plan(who, node_tokens, n_nodes, pred_off, preds, is_final, T, window_nodes, V, blank, post));
  if (lo_force) {
    const int n_launch = (T + slab_rows - 1) / slab_rows, top = std::max(0, (sc.N + 63) / 64 * 64 - sc.W);
    for (int i = 0; i < n_launch; ++i) {
      const int v = lo_force[i];
      if (v % 64 != 0 || v < 0 || v > top || (i == 0 ? v != 0 : v < lo_force[i - 1])) {
        set_error(me + ": lo_force[" + std::to_string(i) + "] = " + std::to_string(v) + " must be a multiple of 64 in [0, " +
                  std::to_string(top) + "], not below the entry before it, and 0 for launch 0");
        return E_ARG;
      }
    }
    sc.lo_force = lo_force;
    sc.n_force = n_launch;
  }
  RVB_TRY(need_gpu());
  Dev dlp;
  const size_t n = (size_t)sc.N;
  std::vector<int32_t> rows((size_t)T);
  for (int t = 0; t < T; ++t) rows[t] = t;
  double ll = 0.0;
  int r = up_raw(dlp, lp, (size_t)T * V * 4);
  if (r == OK) r = sc.begin(nullptr);
  if (r == OK) r = sc.batch(nullptr, rows);
  r = feed_slabs(r, T, slab_rows, false, [&](int r0, int nr) { return sc.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, nr); });
  if (r == OK) r = sc.loglik(nullptr, &ll);
  std::vector<float> vis(n), occ(n), mean(n), peak(n);
  std::vector<int32_t> pf(n);
  if (r == OK && post) {
    r = sc.batch_back(nullptr, rows);
    r = feed_slabs(r, T, slab_rows, true, [&](int r0, int nr) { return sc.advance_back(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, nr); });
    if (r == OK) r = sc.finish(nullptr, vis.data(), occ.data(), mean.data(), peak.data(), pf.data());
  }
  if (r != OK) (void)hipDeviceSynchronize();
  const std::vector<CtcGraphWindowScorer::Launch> launches = sc.launches;
  sc.release();
  RVB_TRY(r);                                      // nothing was written so far: a refusal leaves every output untouched
  *loglik_out = ll;
  for (const auto& m : launches)
    for (int t = m.f0; t < m.f1; ++t) lo_out[t] = m.lo;
  if (best_out)
    for (size_t i = 0; i < launches.size(); ++i) best_out[i] = launches[i].best;
  if (launches_out) *launches_out = (int32_t)launches.size();
  if (visit) memcpy(visit, vis.data(), n * 4);
  if (occupancy) memcpy(occupancy, occ.data(), n * 4);
  if (mean_frame) memcpy(mean_frame, mean.data(), n * 4);
  if (peak_post) memcpy(peak_post, peak.data(), n * 4);
  if (peak_frame) memcpy(peak_frame, pf.data(), n * 4);
  return OK;
}

int rvb_test_ctc_find(const float* lp, const int32_t* T, int n_seq, int V, const float* w, const int32_t* tokens, const int32_t* tok_lens,
                      int n_phrases, const float* threshold, int blank, int slab_rows, int max_candidates, int max_hits,
                      int64_t* raw_count, int32_t* raw_end, int32_t* raw_start, float* raw_score, int32_t* n_hits, int32_t* hit_start,
                      int32_t* hit_end, float* hit_score) {
  const char* who = "rvb_test_ctc_find";
  const std::string me(who);
  if (!lp || !T || !tokens || !tok_lens || !threshold || !raw_count || !raw_end || !raw_start || !raw_score || !n_hits || !hit_start ||
      !hit_end || !hit_score) { set_error(me + ": null argument"); return E_ARG; }
  if (n_phrases < 1 || n_seq < 1) { set_error(me + ": need n_phrases >= 1 and n_seq >= 1"); return E_ARG; }
  if (max_candidates < 1 || max_hits < 1) { set_error(me + ": need max_candidates >= 1 and max_hits >= 1"); return E_ARG; }
  if (slab_rows < 1) { set_error(me + ": need slab_rows >= 1"); return E_ARG; }
  for (int i = 0; i < n_seq; ++i)
    if (T[i] < 0) { set_error(me + ": sequence " + std::to_string(i) + ": negative frame count"); return E_ARG; }
  std::vector<std::vector<int32_t>> rows;
  const int M = (int)lab_rows(T, n_seq, &rows);
  CtcFinder fd;
  RVB_TRY(fd.plan(who, tokens, tok_lens, n_phrases, threshold, rows, V, blank, max_candidates));
  std::vector<float> wmax((size_t)M);
  for (int r = 0; r < M; ++r) {
    float m = w ? w[r] : -INFINITY;
    if (!w) for (int v = 0; v < V; ++v) m = std::max(m, lp[(size_t)r * V + v]);
    if (!std::isfinite(m)) { set_error(me + ": the row maximum of frame " + std::to_string(r) + " is not finite"); return E_ARG; }
    wmax[r] = m;
  }
  RVB_TRY(need_gpu());
  Dev dlp, dw;
  int r = up_raw(dlp, lp, (size_t)M * V * 4);
  if (r == OK) r = up_raw(dw, wmax.data(), (size_t)M * 4);
  if (r == OK) r = fd.begin(nullptr);
  r = feed_slabs(r, M, slab_rows, false, [&](int r0, int n) {
    return fd.advance(nullptr, (const float*)dlp.p + (size_t)r0 * V, V, r0, n, (const float*)dw.p + r0);
  });
  if (r == OK) r = fd.finish(nullptr, max_hits, n_hits, hit_start, hit_end, hit_score, raw_count, raw_end, raw_start, raw_score);
  if (r != OK) (void)hipDeviceSynchronize();
  fd.release();
  return r;
}

int rvb_test_slab_windows(const char* who, const int32_t* rows, const int32_t* T, int n_seq, const int32_t* slabs, int n_slabs,
                          int descending, int32_t* windows_out, int32_t* any_out, int32_t* touches_out, int32_t* fed_out,
                          int32_t* covered_out) {
  if (!who || !rows || !T || !slabs || !windows_out || !any_out || !touches_out || !fed_out || !covered_out || n_seq < 1 || n_slabs < 0) {
    set_error("rvb_test_slab_windows: null argument or no sequence");
    return E_ARG;
  }
  *fed_out = 0; *covered_out = 0;
  std::vector<FindSeq> seq(n_seq, FindSeq{});
  std::vector<int32_t> h_rows;
  int64_t frame_off = 0;
  for (int i = 0; i < n_seq; ++i) {
    if (T[i] < 0) { set_error("rvb_test_slab_windows: negative frame count"); return E_ARG; }
    seq[i].frame_off = (int)frame_off; seq[i].T = T[i];
    seq[i].f0 = seq[i].f1 = descending ? T[i] : 0;            // as begin() / CtcScorer::finish_forward leave them
    const int32_t* rw = rows + frame_off;
    RVB_TRY(slab_take_rows(who, std::string(who) + ": sequence " + std::to_string(i) + ": ", std::vector<int32_t>(rw, rw + T[i]), &h_rows,
                           &frame_off));
  }
  for (int k = 0; k < n_slabs; ++k) {
    const int r0 = slabs[2 * k], nrows = slabs[2 * k + 1];
    touches_out[k] = slab_touches(seq, h_rows, r0, nrows);
    bool any = false;
    RVB_TRY(slab_window(who, descending, seq, h_rows, r0, nrows, &any));
    any_out[k] = any;
    for (int i = 0; i < n_seq; ++i) { windows_out[((size_t)k * n_seq + i) * 2] = seq[i].f0; windows_out[((size_t)k * n_seq + i) * 2 + 1] = seq[i].f1; }
    *fed_out = k + 1;
  }
  RVB_TRY(slab_covered(who, descending, seq));
  *covered_out = 1;
  return OK;
}

int rvb_test_lse_gather_ex(const float* logits, int R, int V, int ld, const int32_t* target, float blank_penalty, int blank_id,
                           float* out) {
  RVB_TRY(rowlse_args("rvb_test_lse_gather_ex", logits, R, V, ld));
  if (!target || !out) { set_error("rvb_test_lse_gather_ex: null target / out"); return E_ARG; }
  for (int r = 0; r < R; ++r) if (target[r] < 0 || target[r] >= V) { set_error("rvb_test_lse_gather_ex: target outside [0, V)"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dl, dt, dout;
  RVB_TRY(up_raw(dl, logits, (size_t)R * ld * 4));
  RVB_TRY(up_raw(dt, target, (size_t)R * 4));
  RVB_TRY(dout.alloc((size_t)R * 4)); RVB_HIP_CHECK(hipMemset(dout.p, 0xff, (size_t)R * 4));
  RVB_TRY(lse_gather(nullptr, (const float*)dl.p, R, V, ld, (const int*)dt.p, (float*)dout.p, blank_penalty, blank_id));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(out, dout.p, (size_t)R * 4, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_lse_gather(const float* logits, int R, int V, const int32_t* target, float* out) {
  return rvb_test_lse_gather_ex(logits, R, V, V, target, 0.f, -1, out);
}

int rvb_test_lse_gather_multi_ex(const float* logits, int R, int V, int ld, const int32_t* ptr, const int32_t* target, float* out) {
  RVB_TRY(rowlse_args("rvb_test_lse_gather_multi_ex", logits, R, V, ld));
  if (!ptr) { set_error("rvb_test_lse_gather_multi_ex: null ptr"); return E_ARG; }
  if (ptr[0] != 0) { set_error("rvb_test_lse_gather_multi_ex: ptr[0] must be 0"); return E_ARG; }
  for (int r = 0; r < R; ++r) if (ptr[r + 1] < ptr[r]) { set_error("rvb_test_lse_gather_multi_ex: ptr decreases"); return E_ARG; }
  const int P = ptr[R];
  if (P > 0 && (!target || !out)) { set_error("rvb_test_lse_gather_multi_ex: targets without target / out arrays"); return E_ARG; }
  for (int p = 0; p < P; ++p) if (target[p] < 0 || target[p] >= V) { set_error("rvb_test_lse_gather_multi_ex: target outside [0, V)"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dl, dp, dt, dout;
  const size_t nout = (size_t)(P > 0 ? P : 1) * 4;
  RVB_TRY(up_raw(dl, logits, (size_t)R * ld * 4));
  RVB_TRY(up_raw(dp, ptr, (size_t)(R + 1) * 4));
  if (P > 0) { RVB_TRY(up_raw(dt, target, (size_t)P * 4)); } else { RVB_TRY(dt.alloc(4)); }
  RVB_TRY(dout.alloc(nout)); RVB_HIP_CHECK(hipMemset(dout.p, 0xff, nout));
  RVB_TRY(lse_gather_multi(nullptr, (const float*)dl.p, R, V, ld, (const int*)dp.p, (const int*)dt.p, (float*)dout.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (P > 0) RVB_HIP_CHECK(hipMemcpy(out, dout.p, (size_t)P * 4, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_lse_gather_multi(const float* logits, int R, int V, const int32_t* ptr, const int32_t* target, int P, float* out) {
  if (ptr && R >= 1 && ptr[R] != P) { set_error("rvb_test_lse_gather_multi: P is not ptr[R]"); return E_ARG; }
  return rvb_test_lse_gather_multi_ex(logits, R, V, V, ptr, target, out);
}

int rvb_test_row_xent(const float* logits, int R, int V, int ld, const int32_t* ptr, const int32_t* target, float* logp, float* lse,
                      double* sum_x, int32_t* top1) {
  if (!logits || !ptr || !lse || !sum_x || !top1 || R < 1 || V < 1 || ld < V) { set_error("rvb_test_row_xent: null argument, R < 1 or not 1 <= V <= ld"); return E_ARG; }
  if (ptr[0] != 0) { set_error("rvb_test_row_xent: ptr[0] must be 0"); return E_ARG; }
  for (int r = 0; r < R; ++r) if (ptr[r + 1] < ptr[r]) { set_error("rvb_test_row_xent: ptr decreases"); return E_ARG; }
  const int P = ptr[R];
  if (P > 0 && (!target || !logp)) { set_error("rvb_test_row_xent: targets without target / logp arrays"); return E_ARG; }
  for (int p = 0; p < P; ++p) if (target[p] < 0 || target[p] >= V) { set_error("rvb_test_row_xent: target outside [0, V)"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dl, dp, dt, dlogp, dlse, dsum, dtop;
  RVB_TRY(up_raw(dl, logits, (size_t)R * ld * 4));
  RVB_TRY(up_raw(dp, ptr, (size_t)(R + 1) * 4));
  if (P > 0) { RVB_TRY(up_raw(dt, target, (size_t)P * 4)); } else { RVB_TRY(dt.alloc(4)); }
  RVB_TRY(dlogp.alloc((size_t)(P > 0 ? P : 1) * 4));
  RVB_TRY(dlse.alloc((size_t)R * 4)); RVB_TRY(dsum.alloc((size_t)R * 8)); RVB_TRY(dtop.alloc((size_t)R * 4));
  RVB_TRY(row_xent(nullptr, (const float*)dl.p, R, V, ld, (const int*)dp.p, (const int*)dt.p, (float*)dlogp.p, (float*)dlse.p,
                 (double*)dsum.p, (int*)dtop.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (P > 0) RVB_HIP_CHECK(hipMemcpy(logp, dlogp.p, (size_t)P * 4, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(lse, dlse.p, (size_t)R * 4, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(sum_x, dsum.p, (size_t)R * 8, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(top1, dtop.p, (size_t)R * 4, hipMemcpyDeviceToHost));
  return OK;
}

// fp8 GEMM of gemm2.hip on host floats: A is quantised per tensor (a_scale), W per output channel, exactly as the engine
// does; a_deq / w_deq (nullable) receive the values the quantised operands stand for, so that the caller's fp64 reference
// isolates the kernel from the quantisation.  out_kind 0 bf16, 1 fp32, 2 fp8 (values are returned de-quantised).
int rvb_test_gemm_fp8(const float* A, const float* W, const float* bias, const float* res, float* C, int M, int N, int K,
                      float a_scale, float alpha, int act, int out_kind, float out_scale, float* a_deq, float* w_deq) {
  RVB_TRY(need_gpu());
  std::vector<uint8_t> qa((size_t)M * K), qw((size_t)N * K);
  std::vector<float> ws(N);
  for (size_t i = 0; i < qa.size(); ++i) { qa[i] = f32_to_fp8_host(A[i] / a_scale); if (a_deq) a_deq[i] = fp8_to_f32_host(qa[i]) * a_scale; }
  for (int n = 0; n < N; ++n) {
    float am = 0.f;
    for (int k = 0; k < K; ++k) am = fmaxf(am, fabsf(W[(size_t)n * K + k]));
    ws[n] = am > 0.f ? am / 448.f : 1.f;
    for (int k = 0; k < K; ++k) {
      qw[(size_t)n * K + k] = f32_to_fp8_host(W[(size_t)n * K + k] / ws[n]);
      if (w_deq) w_deq[(size_t)n * K + k] = fp8_to_f32_host(qw[(size_t)n * K + k]) * ws[n];
    }
  }
  Dev dA, dW, dS, dB, dR, dC;
  RVB_TRY(up_raw(dA, qa.data(), qa.size())); RVB_TRY(up_raw(dW, qw.data(), qw.size())); RVB_TRY(up_raw(dS, ws.data(), (size_t)N * 4));
  RVB_TRY(up_raw(dB, bias, (size_t)N * 4)); RVB_TRY(up_raw(dR, res, (size_t)M * N * 4));
  const size_t osz = out_kind == 1 ? 4 : out_kind == 2 ? 1 : 2;
  RVB_TRY(dC.alloc((size_t)M * N * osz));
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dA.p; g.W = dW.p; g.bias = (const float*)dB.p; g.res = (const float*)dR.p; g.C = dC.p;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N; g.ldres = N; g.alpha = alpha; g.act = act;
  g.out_f32 = out_kind == 1; g.out_fp8 = out_kind == 2; g.in_fp8 = 1; g.a_scale = a_scale; g.w_scale = (const float*)dS.p;
  g.out_inv_scale = 1.f / out_scale;
  RVB_TRY(gemm(nullptr, DT_BF16, g));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (out_kind == 1) return down_T(dC, DT_F32, true, C, (size_t)M * N);
  if (out_kind == 0) return down_T(dC, DT_BF16, false, C, (size_t)M * N);
  std::vector<uint8_t> q((size_t)M * N);
  RVB_HIP_CHECK(hipMemcpy(q.data(), dC.p, q.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < q.size(); ++i) C[i] = fp8_to_f32_host(q[i]) * out_scale;
  return OK;
}

// fp8 implicit-GEMM convolution of conv_gemm.hip (round 4 candidate) on host floats.  x [B][Fi][Ti][Cin] and w [Cout][9][Cin] are
// quantised as the engine would (per tensor / per output channel) and laid out as the kernel wants them (bordered NHWC); x_deq /
// w_deq (nullable) receive the values the quantised operands stand for.  res (nullable) [B][Fo][To][Cout] is rounded to bf16.
// Outputs (either nullable): out [B][Fo][To][Cout] from the kernel's bf16 tensor, out8 the same from its e4m3 tensor (de-quantised
// with out8_scale); *amax receives the running maximum the kernel recorded.
int rvb_test_conv_igemm_fp8(const float* x, const float* w, const float* bias, const float* res, float* out, float* out8, int B,
                            int Fi, int Ti, int Cin, int Cout, int stride, int relu, float a_scale, float out8_scale, float* x_deq,
                            float* w_deq, float* amax) {
  RVB_TRY(need_gpu());
  const int Fo = (Fi - 1) / stride + 1, To = (Ti - 1) / stride + 1;
  const size_t npi = (size_t)B * (Fi + 2) * (Ti + 2) * Cin, npo = (size_t)B * (Fo + 2) * (To + 2) * Cout;
  std::vector<uint8_t> qx(npi, 0), qw((size_t)Cout * 9 * Cin);
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < Fi; ++f)
      for (int t = 0; t < Ti; ++t)
        for (int c = 0; c < Cin; ++c) {
          const size_t si = (((size_t)b * Fi + f) * Ti + t) * Cin + c;
          const uint8_t q = f32_to_fp8_host(x[si] / a_scale);
          qx[(((size_t)b * (Fi + 2) + f + 1) * (Ti + 2) + t + 1) * Cin + c] = q;
          if (x_deq) x_deq[si] = fp8_to_f32_host(q) * a_scale;
        }
  std::vector<float> ws(Cout);
  const size_t K = (size_t)9 * Cin;
  for (int n = 0; n < Cout; ++n) {
    float am = 0.f;
    for (size_t k = 0; k < K; ++k) am = fmaxf(am, fabsf(w[(size_t)n * K + k]));
    ws[n] = am > 0.f ? am / 448.f : 1.f;
    for (size_t k = 0; k < K; ++k) {
      qw[(size_t)n * K + k] = f32_to_fp8_host(w[(size_t)n * K + k] / ws[n]);
      if (w_deq) w_deq[(size_t)n * K + k] = fp8_to_f32_host(qw[(size_t)n * K + k]) * ws[n];
    }
  }
  Dev dx, dw, ds, db, dr, dout, dout8, dam;
  RVB_TRY(up_raw(dx, qx.data(), qx.size())); RVB_TRY(up_raw(dw, qw.data(), qw.size())); RVB_TRY(up_raw(ds, ws.data(), (size_t)Cout * 4));
  RVB_TRY(up_raw(db, bias, (size_t)Cout * 4));
  if (res) {
    std::vector<bf16_t> rb(npo, 0);
    for (int b = 0; b < B; ++b)
      for (int f = 0; f < Fo; ++f)
        for (int t = 0; t < To; ++t)
          for (int c = 0; c < Cout; ++c)
            rb[(((size_t)b * (Fo + 2) + f + 1) * (To + 2) + t + 1) * Cout + c] = f32_to_bf16(res[(((size_t)b * Fo + f) * To + t) * Cout + c]);
    RVB_TRY(up_raw(dr, rb.data(), npo * 2));
  }
  if (out) { RVB_TRY(dout.alloc(npo * 2)); RVB_HIP_CHECK(hipMemset(dout.p, 0, npo * 2)); }
  if (out8) { RVB_TRY(dout8.alloc(npo)); RVB_HIP_CHECK(hipMemset(dout8.p, 0, npo)); }
  RVB_TRY(dam.alloc(4)); RVB_HIP_CHECK(hipMemset(dam.p, 0, 4));
  ConvArgs a{};
  a.bias = (const float*)db.p; a.res = dr.p; a.out = dout.p;
  a.B = B; a.Fi = Fi; a.Ti = Ti; a.Cin = Cin; a.Fo = Fo; a.To = To; a.Cout = Cout; a.stride = stride; a.taps = 9; a.relu = relu;
  a.in8 = dx.p; a.w8 = dw.p; a.w8_scale = (const float*)ds.p; a.a_scale = a_scale; a.out8 = dout8.p; a.out8_inv_scale = 1.f / out8_scale;
  a.amax8 = (unsigned*)dam.p;
  if (!conv_igemm8_applicable(DT_BF16, a)) { set_error("rvb_test_conv_igemm_fp8: shape not supported (channels multiples of 128, 3x3, stride 1 | 2)"); return E_ARG; }
  RVB_TRY(conv_igemm8(nullptr, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (amax) RVB_HIP_CHECK(hipMemcpy(amax, dam.p, 4, hipMemcpyDeviceToHost));
  if (out) {
    std::vector<bf16_t> ob(npo);
    RVB_HIP_CHECK(hipMemcpy(ob.data(), dout.p, npo * 2, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
      for (int f = 0; f < Fo; ++f)
        for (int t = 0; t < To; ++t)
          for (int c = 0; c < Cout; ++c)
            out[(((size_t)b * Fo + f) * To + t) * Cout + c] = bf16_to_f32(ob[(((size_t)b * (Fo + 2) + f + 1) * (To + 2) + t + 1) * Cout + c]);
  }
  if (out8) {
    std::vector<uint8_t> o8(npo);
    RVB_HIP_CHECK(hipMemcpy(o8.data(), dout8.p, npo, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
      for (int f = 0; f < Fo; ++f)
        for (int t = 0; t < To; ++t)
          for (int c = 0; c < Cout; ++c)
            out8[(((size_t)b * Fo + f) * To + t) * Cout + c] = fp8_to_f32_host(o8[(((size_t)b * (Fo + 2) + f + 1) * (To + 2) + t + 1) * Cout + c]) * out8_scale;
  }
  return OK;
}

// LayerNorm with fp8 outputs (first stage and / or the fused second LayerNorm); results returned de-quantised
int rvb_test_rownorm_fp8(const float* x, const float* gamma, const float* beta, float eps, int silu, int M, int d, float scale,
                         float* out, const float* gamma2, const float* beta2, float eps2, float scale2, float* out1_f32, float* out2) {
  RVB_TRY(need_gpu());
  Dev dx, dg, db, dg2, db2, dout, dout2;
  RVB_TRY(up_raw(dx, x, (size_t)M * d * 4)); RVB_TRY(up_raw(dg, gamma, (size_t)d * 4)); RVB_TRY(up_raw(db, beta, (size_t)d * 4));
  RVB_TRY(up_raw(dg2, gamma2, (size_t)d * 4)); RVB_TRY(up_raw(db2, beta2, (size_t)d * 4));
  NormArgs a;
  a.x = (const float*)dx.p; a.gamma = (const float*)dg.p; a.beta = (const float*)db.p; a.eps = eps; a.mode = NORM_LN; a.silu = silu;
  a.add = nullptr; a.M = M; a.d = d;
  const bool two = gamma2 != nullptr;
  if (two) {       // stage 1 fp32 (in place semantics of norm_final), stage 2 fp8
    RVB_TRY(dout.alloc((size_t)M * d * 4)); RVB_TRY(dout2.alloc((size_t)M * d));
    a.out = dout.p; a.out_f32 = 1; a.gamma2 = (const float*)dg2.p; a.beta2 = (const float*)db2.p; a.eps2 = eps2; a.out2 = dout2.p;
    a.out2_fp8 = 1; a.out2_inv_scale = 1.f / scale2;
  } else {
    RVB_TRY(dout.alloc((size_t)M * d));
    a.out = dout.p; a.out_f32 = 0; a.out_fp8 = 1; a.out_inv_scale = 1.f / scale;
  }
  RVB_TRY(rownorm(nullptr, DT_BF16, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  std::vector<uint8_t> q((size_t)M * d);
  if (two) {
    RVB_HIP_CHECK(hipMemcpy(out1_f32, dout.p, (size_t)M * d * 4, hipMemcpyDeviceToHost));
    RVB_HIP_CHECK(hipMemcpy(q.data(), dout2.p, q.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < q.size(); ++i) out2[i] = fp8_to_f32_host(q[i]) * scale2;
  } else {
    RVB_HIP_CHECK(hipMemcpy(q.data(), dout.p, q.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < q.size(); ++i) out[i] = fp8_to_f32_host(q[i]) * scale;
  }
  return OK;
}

// e4m3 byte -> float at `scale`; the two NaN codes (what the hooks below pre-fill fp8 outputs with) stay NaN
static float fp8_deq_or_nan(uint8_t q, float scale) {
  return (q & 0x7f) == 0x7f ? __builtin_nanf("") : fp8_to_f32_host(q) * scale;
}
static int down_fp8(const Dev& d, float* dst, size_t n, float scale) {
  std::vector<uint8_t> q(n);
  RVB_HIP_CHECK(hipMemcpy(q.data(), d.p, n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) dst[i] = fp8_deq_or_nan(q[i], scale);
  return OK;
}

// gemm() with the whole of GemmArgs but the row-periodic addend (test_api.h): the GemmArgs are filled as run_gemm fills them
int rvb_test_gemm_ex(rvb_test_gemm_args* t) {
  auto bad = [](const char* m) { set_error(std::string("rvb_test_gemm_ex: ") + m); return E_ARG; };
  if (!t) return bad("null");
  t->path = 0;
  const int dtype = t->dtype;
  if (!t->A || !t->W || !t->C || (dtype != DT_F32 && dtype != DT_BF16)) return bad("null A, W or C, or an unknown dtype");
  const int M = t->M, N = t->N, K = t->K;
  if (M < 0 || N < 1 || K < 1 || t->a_row0 < 0) return bad("M < 0, N < 1, K < 1 or a negative a_row0");
  const int lda = t->conv ? t->cC : t->lda;
  const int c_rows = t->c_rows ? t->c_rows : M;
  if (lda < 1 || t->ldw < K || t->ldc < N || c_rows < M) return bad("lda < 1, ldw < K, ldc < N or c_rows < M");
  if (t->in_fp8 && (dtype != DT_BF16 || !(t->a_scale > 0.f) || t->conv)) return bad("fp8 operands: bf16 engine, a positive a_scale, no convolution gather");
  if (t->out_fp8 && (!t->in_fp8 || !(t->out_scale > 0.f))) return bad("an fp8 output needs fp8 operands and a positive scale");
  const bool f32out = !t->out_fp8 && (dtype == DT_F32 || t->out_f32);
  if (t->inplace && (t->res || !f32out)) return bad("inplace: the fp32 output buffer is the residual (res must be null)");
  if (t->res && t->ldres < N) return bad("ldres < N");
  size_t a_elems = (size_t)(t->a_elems > 0 ? t->a_elems : 0);
  if (t->conv) {
    const int T2 = (t->cT1 - 3) / 2 + 1, F2 = (t->cF1 - 3) / 2 + 1;
    if (t->cT1 < 3 || t->cF1 < 3 || t->cC < 1 || t->cB < 1 || M != t->cB * T2 * F2 || K != 9 * t->cC || t->a_row0 != 0) return bad("conv shape mismatch");
    a_elems = (size_t)t->cB * t->cT1 * t->cF1 * t->cC;
  } else if (M > 0 && (int64_t)a_elems < ((int64_t)t->a_row0 + M - 1) * lda + K) {
    return bad("a_elems < (a_row0 + M - 1) * lda + K");
  }
  RVB_TRY(need_gpu());
  const size_t w_elems = (size_t)N * t->ldw, c_elems = (size_t)c_rows * t->ldc;
  Dev dA, dW, dS, dB, dR, dC;
  if (t->in_fp8) {      // A per tensor, W per output channel over its K columns (rvb_test_gemm_fp8); pad columns of W are zero bytes
    std::vector<uint8_t> qa(a_elems), qw(w_elems, 0);
    std::vector<float> ws(N);
    for (size_t i = 0; i < a_elems; ++i) { qa[i] = f32_to_fp8_host(t->A[i] / t->a_scale); if (t->a_deq) t->a_deq[i] = fp8_to_f32_host(qa[i]) * t->a_scale; }
    for (int n = 0; n < N; ++n) {
      const float* w = t->W + (size_t)n * t->ldw;
      float am = 0.f;
      for (int k = 0; k < K; ++k) am = fmaxf(am, fabsf(w[k]));
      ws[n] = am > 0.f ? am / 448.f : 1.f;
      for (int k = 0; k < t->ldw; ++k) {
        const uint8_t q = k < K ? f32_to_fp8_host(w[k] / ws[n]) : 0;
        qw[(size_t)n * t->ldw + k] = q;
        if (t->w_deq) t->w_deq[(size_t)n * t->ldw + k] = fp8_to_f32_host(q) * ws[n];
      }
    }
    if (a_elems > 0) RVB_TRY(up_raw(dA, qa.data(), a_elems)); else RVB_TRY(dA.alloc(16));
    RVB_TRY(up_raw(dW, qw.data(), qw.size()));
    RVB_TRY(up_raw(dS, ws.data(), (size_t)N * 4));
  } else {
    if (a_elems > 0) RVB_TRY(up_T(dA, dtype, t->A, a_elems)); else RVB_TRY(dA.alloc(16));
    RVB_TRY(up_T(dW, dtype, t->W, w_elems));
  }
  RVB_TRY(up_raw(dB, t->bias, (size_t)N * 4));
  if (M > 0) RVB_TRY(up_raw(dR, t->res, (size_t)M * t->ldres * 4));
  // the caller's C in the output's own format: canaries and an in-place residual survive the way up
  if (t->out_fp8) {
    std::vector<uint8_t> q(c_elems);
    for (size_t i = 0; i < c_elems; ++i) q[i] = t->C[i] != t->C[i] ? 0x7f : f32_to_fp8_host(t->C[i] / t->out_scale);
    if (c_elems > 0) RVB_TRY(up_raw(dC, q.data(), c_elems)); else RVB_TRY(dC.alloc(16));
  } else if (c_elems > 0) {
    RVB_TRY(up_T(dC, f32out ? DT_F32 : DT_BF16, t->C, c_elems));
  } else {
    RVB_TRY(dC.alloc(16));
  }
  const size_t a_esz = t->in_fp8 ? 1 : dt_size(dtype);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = (const char*)dA.p + (size_t)t->a_row0 * lda * a_esz; g.W = dW.p; g.bias = (const float*)dB.p; g.C = dC.p;
  g.res = t->inplace ? (const float*)dC.p : (const float*)dR.p;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = t->ldw; g.ldc = t->ldc; g.ldres = t->inplace ? t->ldc : t->ldres;
  g.alpha = t->alpha; g.act = t->act; g.out_f32 = t->out_f32 ? 1 : 0;
  if (t->conv) {
    g.conv = 1; g.cT1 = t->cT1; g.cF1 = t->cF1; g.cT2 = (t->cT1 - 3) / 2 + 1; g.cF2 = (t->cF1 - 3) / 2 + 1; g.cC = t->cC;
  }
  if (t->in_fp8) { g.in_fp8 = 1; g.a_scale = t->a_scale; g.w_scale = (const float*)dS.p; }
  if (t->out_fp8) { g.out_fp8 = 1; g.out_inv_scale = 1.f / t->out_scale; }
  // where gemm() sends it (gemm.hip: ACT_GLU and fp8 operands exist on gemm2.hip only; otherwise the variant switch and gemm2_applicable)
  t->path = (t->act == ACT_GLU || t->in_fp8 || (g_gemm_variant != 1 && (dtype == DT_BF16 || g_gemm_variant == 2) && gemm2_applicable(dtype, g))) ? 2 : 1;
  RVB_TRY(gemm(nullptr, dtype, g));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (c_elems == 0) return OK;
  if (t->out_fp8) return down_fp8(dC, t->C, c_elems, t->out_scale);
  return down_T(dC, f32out ? DT_F32 : DT_BF16, f32out, t->C, c_elems);
}

// rownorm() with the whole of NormArgs (test_api.h)
int rvb_test_rownorm_ex(rvb_test_norm_args* t) {
  if (!t || !t->x || !t->gamma || !t->beta || !t->out || t->M < 1 || t->d < 1 || (t->dtype != DT_F32 && t->dtype != DT_BF16)) {
    set_error("rvb_test_rownorm_ex: null argument, M < 1, d < 1 or an unknown dtype"); return E_ARG;
  }
  const bool two = t->gamma2 != nullptr;
  if (two && (!t->beta2 || !t->out2)) { set_error("rvb_test_rownorm_ex: the second stage needs gamma2, beta2 and out2"); return E_ARG; }
  if ((t->out_fp8 && !(t->out_scale > 0.f)) || (two && t->out2_fp8 && !(t->out2_scale > 0.f))) {
    set_error("rvb_test_rownorm_ex: an fp8 output needs a positive scale"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  const int dtype = t->dtype;
  const size_t n = (size_t)t->M * t->d;
  Dev dx, dg, db, da, dg2, db2, dout, dout2, dsat;
  if (t->x_bf16) RVB_TRY(up_T(dx, DT_BF16, t->x, n)); else RVB_TRY(up_raw(dx, t->x, n * 4));
  RVB_TRY(up_raw(dg, t->gamma, (size_t)t->d * 4)); RVB_TRY(up_raw(db, t->beta, (size_t)t->d * 4));
  RVB_TRY(up_T(da, dtype, t->add, n));
  RVB_TRY(up_raw(dg2, t->gamma2, (size_t)t->d * 4)); RVB_TRY(up_raw(db2, t->beta2, (size_t)t->d * 4));
  // four bytes per element whatever the output type (a call the launcher is going to refuse may name any combination)
  RVB_TRY(dout.alloc(n * 4)); RVB_HIP_CHECK(hipMemset(dout.p, 0xff, n * 4));
  if (two) { RVB_TRY(dout2.alloc(n * 4)); RVB_HIP_CHECK(hipMemset(dout2.p, 0xff, n * 4)); }
  RVB_TRY(dsat.alloc(8)); RVB_HIP_CHECK(hipMemset(dsat.p, 0, 8));
  NormArgs a;
  a.x = (const float*)dx.p; a.x_bf16 = t->x_bf16 ? 1 : 0; a.gamma = (const float*)dg.p; a.beta = (const float*)db.p; a.eps = t->eps;
  a.mode = t->mode; a.silu = t->silu; a.add = da.p; a.out = dout.p; a.out_f32 = t->out_f32; a.M = t->M; a.d = t->d;
  a.out_fp8 = t->out_fp8 ? 1 : 0;
  if (t->out_fp8) a.out_inv_scale = 1.f / t->out_scale;
  if (two) {
    a.gamma2 = (const float*)dg2.p; a.beta2 = (const float*)db2.p; a.eps2 = t->eps2; a.out2 = dout2.p;
    a.out2_fp8 = t->out2_fp8 ? 1 : 0;
    if (t->out2_fp8) a.out2_inv_scale = 1.f / t->out2_scale;
  }
  a.sat = (unsigned*)dsat.p; a.sat2 = (unsigned*)dsat.p + 1;
  RVB_TRY(rownorm(nullptr, dtype, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  uint32_t sats[2];
  RVB_HIP_CHECK(hipMemcpy(sats, dsat.p, 8, hipMemcpyDeviceToHost));
  t->sat = sats[0]; t->sat2 = sats[1];
  if (t->out_fp8) RVB_TRY(down_fp8(dout, t->out, n, t->out_scale));
  else RVB_TRY(down_T(dout, dtype, t->out_f32 != 0, t->out, n));
  if (two) {
    if (t->out2_fp8) RVB_TRY(down_fp8(dout2, t->out2, n, t->out2_scale));
    else RVB_TRY(down_T(dout2, dtype, false, t->out2, n));
  }
  return OK;
}

// subsample_conv1 with its fp8 output, running maximum and saturation counter (test_api.h)
int rvb_test_conv1_ex(int dtype, const float* feats, const float* mean, const float* istd, const float* w, const float* b, float* out,
                      int B, int T0, int F0, int d, float out_fp8_scale, float* amax, uint32_t* sat) {
  if (!feats || !mean || !istd || !w || !b || !out || B < 1 || T0 < 3 || F0 < 3 || d < 1 || (dtype != DT_F32 && dtype != DT_BF16)) {
    set_error("rvb_test_conv1_ex: null argument, B < 1, fewer than 3 frames or bins, d < 1 or an unknown dtype"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  const int T1 = (T0 - 3) / 2 + 1, F1 = (F0 - 3) / 2 + 1;
  Dev df, dm, di, dw, db, dout, dslot;
  RVB_TRY(up_raw(df, feats, (size_t)B * T0 * F0 * 4));
  RVB_TRY(up_raw(dm, mean, (size_t)F0 * 4));
  RVB_TRY(up_raw(di, istd, (size_t)F0 * 4));
  std::vector<float> wt((size_t)d * 9);            // [d][1][3][3] -> tap-major [9][d]
  for (int c = 0; c < d; ++c)
    for (int k = 0; k < 9; ++k) wt[(size_t)k * d + c] = w[(size_t)c * 9 + k];
  RVB_TRY(up_raw(dw, wt.data(), (size_t)d * 9 * 4));
  RVB_TRY(up_raw(db, b, (size_t)d * 4));
  const size_t n = (size_t)B * T1 * F1 * d;
  RVB_TRY(dout.alloc(n * 4)); RVB_HIP_CHECK(hipMemset(dout.p, 0xff, n * 4));
  uint32_t slots[2] = {0, 0};                      // {amax as float bits, sat}
  if (amax) memcpy(&slots[0], amax, 4);
  RVB_TRY(up_raw(dslot, slots, 8));
  RVB_TRY(subsample_conv1(nullptr, dtype, (const float*)df.p, (const float*)dm.p, (const float*)di.p, (const float*)dw.p,
                        (const float*)db.p, dout.p, B, T0, F0, d, out_fp8_scale, amax ? (unsigned*)dslot.p : nullptr,
                        sat ? (unsigned*)dslot.p + 1 : nullptr));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(slots, dslot.p, 8, hipMemcpyDeviceToHost));
  if (amax) memcpy(amax, &slots[0], 4);
  if (sat) *sat = slots[1];
  if (out_fp8_scale > 0.f) return down_fp8(dout, out, n, out_fp8_scale);
  return down_T(dout, dtype, false, out, n);
}

int rvb_test_embed(const float* E, int vocab, const float* pe, int n_pos, const int32_t* tok, const int32_t* pos, float* out, int rows,
                   int d, float scale) {
  if (!E || !pe || !tok || !pos || !out || vocab < 1 || n_pos < 1 || rows < 1 || d < 1) { set_error("rvb_test_embed: null argument or an empty table"); return E_ARG; }
  for (int r = 0; r < rows; ++r)
    if (tok[r] < 0 || tok[r] >= vocab || pos[r] < 0 || pos[r] >= n_pos) { set_error("rvb_test_embed: index outside its table"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dE, dp, dt, dq, dout;
  RVB_TRY(up_raw(dE, E, (size_t)vocab * d * 4)); RVB_TRY(up_raw(dp, pe, (size_t)n_pos * d * 4));
  RVB_TRY(up_raw(dt, tok, (size_t)rows * 4)); RVB_TRY(up_raw(dq, pos, (size_t)rows * 4));
  RVB_TRY(up_raw(dout, out, (size_t)rows * d * 4));
  RVB_TRY(embed_tokens(nullptr, (const float*)dE.p, (const float*)dp.p, (const int*)dt.p, (const int*)dq.p, (float*)dout.p, rows, d, scale));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(out, dout.p, (size_t)rows * d * 4, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_amax_abs(int dtype, const float* x, int64_t n, float* slot) {
  if (!x || !slot || n < 1 || (dtype != DT_F32 && dtype != DT_BF16)) { set_error("rvb_test_amax_abs: null argument, n < 1 or an unknown dtype"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dx, ds;
  RVB_TRY(up_T(dx, dtype, x, (size_t)n));
  RVB_TRY(up_raw(ds, slot, 4));
  RVB_TRY(amax_abs(nullptr, dtype, dx.p, (size_t)n, (float*)ds.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(slot, ds.p, 4, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_convert_f32(int dtype, const float* src, float* dst, int64_t n) {
  if (!src || !dst || n < 1 || (dtype != DT_F32 && dtype != DT_BF16)) { set_error("rvb_test_convert_f32: null argument, n < 1 or an unknown dtype"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev ds, dd;
  RVB_TRY(up_raw(ds, src, (size_t)n * 4));
  RVB_TRY(dd.alloc((size_t)n * 4)); RVB_HIP_CHECK(hipMemset(dd.p, 0xff, (size_t)n * 4));
  RVB_TRY(convert_f32(nullptr, dtype, (const float*)ds.p, dd.p, (size_t)n));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dd, dtype, false, dst, (size_t)n);
}

int rvb_test_gather_cache(const void* src, void* dst, const int32_t* parent, int R, int L, int rows, int row_bytes) {
  if (!src || !dst || !parent || R < 1 || L < 1 || rows < 0 || rows > L || row_bytes < 1) { set_error("rvb_test_gather_cache: null argument or not 0 <= rows <= L"); return E_ARG; }
  for (int r = 0; r < R; ++r)
    if (parent[r] < 0 || parent[r] >= R) { set_error("rvb_test_gather_cache: parent outside [0, R)"); return E_ARG; }
  RVB_TRY(need_gpu());
  const size_t bytes = (size_t)R * L * row_bytes;
  Dev ds, dd, dp;
  RVB_TRY(up_raw(ds, src, bytes)); RVB_TRY(up_raw(dd, dst, bytes)); RVB_TRY(up_raw(dp, parent, (size_t)R * 4));
  RVB_TRY(gather_cache(nullptr, ds.p, dd.p, (const int*)dp.p, R, L, rows, row_bytes));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(dst, dd.p, bytes, hipMemcpyDeviceToHost));
  return OK;
}

int rvb_test_gather_pairs(const float* table, int rows, int64_t ld, const int32_t* row, const int32_t* col, int n, float* out) {
  if (!table || rows < 1 || ld < 1 || n < 0 || (n > 0 && (!row || !col || !out))) { set_error("rvb_test_gather_pairs: null argument or an empty table"); return E_ARG; }
  for (int i = 0; i < n; ++i)
    if (row[i] < 0 || row[i] >= rows || col[i] < 0 || col[i] >= ld) { set_error("rvb_test_gather_pairs: pair outside the table"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dt, dr, dc, dout;
  RVB_TRY(up_raw(dt, table, (size_t)rows * ld * 4));
  if (n > 0) { RVB_TRY(up_raw(dr, row, (size_t)n * 4)); RVB_TRY(up_raw(dc, col, (size_t)n * 4)); RVB_TRY(up_raw(dout, out, (size_t)n * 4)); }
  RVB_TRY(gather_pairs(nullptr, (const float*)dt.p, (size_t)ld, (const int*)dr.p, (const int*)dc.p, n, (float*)dout.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (n > 0) RVB_HIP_CHECK(hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return OK;
}

// host only: the joint_decoding state machine (search.cpp: JointSearch), driven frame by frame by a caller that supplies the
// attention log-probs -- the CPU tests do that with the oracle's decoder, the engine with its own (rvb_joint_decode)
void* rvb_test_joint_new(int beam, int pre_beam, int blank, int sos, double w_ctc, double w_dec, double bonus) {
  JointParams p;
  p.beam = beam; p.pre_beam = pre_beam; p.blank = blank; p.sos = sos; p.w_ctc = w_ctc; p.w_dec = w_dec; p.bonus = bonus;
  return new JointSearch(p);
}
void rvb_test_joint_free(void* h) { delete (JointSearch*)h; }
// -> 0 frame skipped, 1 processed.  decode[n_decode] = nodes whose decoder row is needed, pairs (pair_node[i], pair_tok[i])
int rvb_test_joint_begin(void* h, int t, const float* tv, const int32_t* ti, int K, float p_tok0, float p_blank, int32_t* decode,
                         int32_t* n_decode, int32_t* pair_node, int32_t* pair_tok, int32_t* n_pairs, int cap) {
  if (!h || !tv || !ti || !n_decode || !n_pairs) { set_error("rvb_test_joint_begin: bad argument"); return E_ARG; }
  std::vector<int> d, pn, pt;
  const bool ran = ((JointSearch*)h)->begin_frame(t, tv, (const int*)ti, K, p_tok0, p_blank, &d, &pn, &pt);
  if ((int)d.size() > cap || (int)pn.size() > cap) { set_error("rvb_test_joint_begin: capacity"); return E_ARG; }
  *n_decode = (int32_t)d.size(); *n_pairs = (int32_t)pn.size();
  for (size_t i = 0; i < d.size(); ++i) decode[i] = d[i];
  for (size_t i = 0; i < pn.size(); ++i) { pair_node[i] = pn[i]; pair_tok[i] = pt[i]; }
  return ran ? 1 : 0;
}
int rvb_test_joint_finish(void* h, const float* vals) {
  if (!h) { set_error("rvb_test_joint_finish: bad argument"); return E_ARG; }
  ((JointSearch*)h)->finish_frame(vals);
  return OK;
}
int rvb_test_joint_prefix(void* h, int node, int32_t* toks, int32_t* n) {
  if (!h || !toks || !n) { set_error("rvb_test_joint_prefix: bad argument"); return E_ARG; }
  std::vector<int> t;
  ((JointSearch*)h)->prefix(node, &t);
  *n = (int32_t)t.size();
  for (size_t i = 0; i < t.size(); ++i) toks[i] = t[i];
  return OK;
}
int rvb_test_joint_result(void* h, int32_t* tokens, int32_t* times, int32_t* end_times, double* conf, int32_t* n, double* score) {
  if (!h || !n || !score) { set_error("rvb_test_joint_result: bad argument"); return E_ARG; }
  JointResult r;
  ((JointSearch*)h)->result(&r);
  *n = (int32_t)r.tokens.size(); *score = r.score;
  for (size_t i = 0; i < r.tokens.size(); ++i) { tokens[i] = r.tokens[i]; times[i] = r.times[i]; end_times[i] = r.end_times[i]; conf[i] = r.tokens_confidence[i]; }
  return OK;
}

int rvb_test_prefix_beam(const float* topk_val, const int32_t* topk_idx, int T, int beam, int blank, int32_t* n_hyps,
                         int32_t* tokens, int32_t* lens, int32_t* times, int32_t* times_lens, double* scores) {
  if (!topk_val || !topk_idx || !n_hyps || T < 0 || beam < 1) { set_error("rvb_test_prefix_beam: bad argument"); return E_ARG; }
  PrefixResult pr;
  prefix_beam_search(topk_val, topk_idx, T, beam, beam, blank, &pr);
  *n_hyps = (int32_t)pr.nbest.size();
  const int ml = T > 0 ? T : 1;
  for (size_t i = 0; i < pr.nbest.size(); ++i) {
    if (lens) lens[i] = (int32_t)pr.nbest[i].size();
    if (times_lens) times_lens[i] = (int32_t)pr.times[i].size();
    if (scores) scores[i] = pr.scores[i];
    for (int j = 0; j < ml; ++j) {
      if (tokens) tokens[i * ml + j] = j < (int)pr.nbest[i].size() ? pr.nbest[i][j] : -1;
      if (times) times[i * ml + j] = j < (int)pr.times[i].size() ? pr.times[i][j] : -1;
    }
  }
  return OK;
}

int rvb_test_prefix_beam_context(const float* topk_val, const int32_t* topk_idx, int T, int beam, int blank, int vocab,
                                 const int32_t* phrase_tokens, const int32_t* phrase_lens, int n_phrases, double context_score,
                                 int32_t* n_hyps, int32_t* tokens, int32_t* lens, int32_t* times, int32_t* times_lens, double* scores,
                                 double* context_scores) {
  if (!topk_val || !topk_idx || !n_hyps || T < 0 || beam < 1) { set_error("rvb_test_prefix_beam_context: bad argument"); return E_ARG; }
  const int np = n_phrases < 0 ? 0 : n_phrases;
  const std::string bad = ContextGraph::check(phrase_tokens, phrase_lens, np, vocab, blank);
  if (!bad.empty()) { set_error("rvb_test_prefix_beam_context: " + bad); return E_ARG; }
  PrefixResult pr;
  if (n_phrases < 0) {
    prefix_beam_search(topk_val, topk_idx, T, beam, beam, blank, &pr);
  } else {
    const ContextGraph graph(phrase_tokens, phrase_lens, np, context_score);
    prefix_beam_search(topk_val, topk_idx, T, beam, beam, blank, &pr, &graph);
  }
  *n_hyps = (int32_t)pr.nbest.size();
  const int ml = T > 0 ? T : 1;
  for (size_t i = 0; i < pr.nbest.size(); ++i) {
    if (lens) lens[i] = (int32_t)pr.nbest[i].size();
    if (times_lens) times_lens[i] = (int32_t)pr.times[i].size();
    if (scores) scores[i] = pr.scores[i];
    if (context_scores) context_scores[i] = n_phrases < 0 ? 0.0 : pr.context_scores[i];
    for (int j = 0; j < ml; ++j) {
      if (tokens) tokens[i * ml + j] = j < (int)pr.nbest[i].size() ? pr.nbest[i][j] : -1;
      if (times) times[i * ml + j] = j < (int)pr.times[i].size() ? pr.times[i][j] : -1;
    }
  }
  return OK;
}

int rvb_test_context_walk(const int32_t* phrase_tokens, const int32_t* phrase_lens, int n_phrases, double context_score, int vocab,
                          int blank, const int32_t* stream, int n_steps, int32_t* num_nodes, double* step_scores, int32_t* step_nodes,
                          double* final_scores) {
  if (n_steps < 0 || (n_steps > 0 && !stream)) { set_error("rvb_test_context_walk: bad argument"); return E_ARG; }
  const std::string bad = ContextGraph::check(phrase_tokens, phrase_lens, n_phrases, vocab, blank);
  if (!bad.empty()) { set_error("rvb_test_context_walk: " + bad); return E_ARG; }
  const ContextGraph graph(phrase_tokens, phrase_lens, n_phrases, context_score);
  if (num_nodes) *num_nodes = graph.num_nodes();
  int state = 0, root;
  for (int i = 0; i < n_steps; ++i) {
    const double sc = graph.forward_one_step(state, stream[i], &state);
    if (step_scores) step_scores[i] = sc;
    if (step_nodes) step_nodes[i] = state;
    if (final_scores) final_scores[i] = graph.finalize(state, &root);
  }
  return OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// GEMM micro-benchmark: random operands generated on the device, `variant` timed with HIP events,
// result compared against the gemm.hip kernel (variant 1) on sampled rows.
// ------------------------------------------------------------------------------------------------
namespace {
template <typename T>
__global__ void fill_random(T* p, size_t n, unsigned seed, float scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)i * 2654435761u ^ seed;
    x ^= x >> 16; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
    p[i] = Cvt<T>::from_f32(((float)(x & 0xffffff) / 8388608.0f - 1.0f) * scale);
  }
}
template <typename T> void fill(void* p, size_t n, unsigned seed, float scale) {
  hipLaunchKernelGGL(fill_random<T>, dim3(2048), dim3(256), 0, nullptr, (T*)p, n, seed, scale);
}
}  // namespace

extern "C" int rvb_test_set_gemm_variant(int v) { g_gemm_variant = v; return OK; }
extern "C" int rvb_test_set_gemm2_opts(int flags, int group_m) { g_gemm2_flags = flags; g_gemm2_group_m = group_m; return OK; }

// per-workgroup phase timestamps of one bf16 gemm2 launch (scripts/gemm_timeline.py): out[6 * wg + {0..3}] = start / stage 0
// landed / main loop done / stores drained (10 ns ticks of the constant clock), [4] = HW_ID, [5] = XCC_ID
extern "C" int rvb_test_gemm_timeline(int M, int N, int K, int act, int out_f32, int with_res, long long* out, int cap, int* n_wg) {
  RVB_TRY(need_gpu());
  Dev dA, dW, dB, dR, dC, dT;
  RVB_TRY(dA.alloc((size_t)M * K * 2)); RVB_TRY(dW.alloc((size_t)N * K * 2)); RVB_TRY(dB.alloc((size_t)N * 4));
  const int padc = getenv("RVB_BENCH_PADC") ? atoi(getenv("RVB_BENCH_PADC")) : 0;      // probe: output / residual row stride off the power of two
  const int ldc = N + padc;
  RVB_TRY(dR.alloc((size_t)M * ldc * 4)); RVB_TRY(dC.alloc((size_t)M * ldc * (out_f32 ? 4 : 2)));
  fill<bf16_t>(dA.p, (size_t)M * K, 1u, 1.0f); fill<bf16_t>(dW.p, (size_t)N * K, 2u, 1.0f / sqrtf((float)K));
  fill<float>(dB.p, N, 3u, 1.0f); fill<float>(dR.p, (size_t)M * ldc, 4u, 1.0f);
  const int wgs = ((M + 255) / 256) * ((N + 255) / 256);
  if (wgs > cap) { set_error("rvb_test_gemm_timeline: output too small"); return E_ARG; }
  RVB_TRY(dT.alloc((size_t)wgs * 6 * 8));
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dA.p; g.W = dW.p; g.bias = (const float*)dB.p; g.res = with_res ? (const float*)dR.p : nullptr; g.C = dC.p;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = ldc; g.ldres = ldc; g.alpha = 0.5f; g.act = act; g.out_f32 = out_f32;
  if (!gemm2_applicable(DT_BF16, g)) { set_error("rvb_test_gemm_timeline: shape not handled by gemm2"); return E_ARG; }
  for (int i = 0; i < 3; ++i) RVB_TRY(gemm2(nullptr, DT_BF16, g));
  g.dbg = (long long*)dT.p;
  RVB_TRY(gemm2(nullptr, DT_BF16, g));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(out, dT.p, (size_t)wgs * 6 * 8, hipMemcpyDeviceToHost));
  *n_wg = wgs;
  return OK;
}

extern "C" int rvb_test_gemm_bench(int dtype, int M, int N, int K, int variant, int iters, int act, int out_f32,
                                   int with_res, double* ms_out, double* max_abs_diff) {
  RVB_TRY(need_gpu());
  Dev dA, dW, dB, dR, dC, dC1;
  const size_t es = dt_size(dtype);
  const bool f32out = dtype == DT_F32 || out_f32;
  // RVB_BENCH_PAD=<elements>: pad the leading dimensions of A and W (probe for channel camping of 2^n row strides)
  const int pad = getenv("RVB_BENCH_PAD") ? atoi(getenv("RVB_BENCH_PAD")) : 0;
  const int ldk = K + pad;
  RVB_TRY(dA.alloc((size_t)M * ldk * es)); RVB_TRY(dW.alloc((size_t)N * ldk * es)); RVB_TRY(dB.alloc((size_t)N * 4));
  RVB_TRY(dR.alloc((size_t)M * N * 4)); RVB_TRY(dC.alloc((size_t)M * N * (f32out ? 4 : 2)));
  RVB_TRY(dC1.alloc((size_t)M * N * (f32out ? 4 : 2)));
  if (dtype == DT_BF16) { fill<bf16_t>(dA.p, (size_t)M * ldk, 1u, 1.0f); fill<bf16_t>(dW.p, (size_t)N * ldk, 2u, 1.0f / sqrtf((float)K)); }
  else { fill<float>(dA.p, (size_t)M * ldk, 1u, 1.0f); fill<float>(dW.p, (size_t)N * ldk, 2u, 1.0f / sqrtf((float)K)); }
  fill<float>(dB.p, N, 3u, 1.0f);
  fill<float>(dR.p, (size_t)M * N, 4u, 1.0f);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dA.p; g.W = dW.p; g.bias = (const float*)dB.p; g.res = with_res ? (const float*)dR.p : nullptr; g.C = dC.p;
  g.M = M; g.N = N; g.K = K; g.lda = ldk; g.ldw = ldk; g.ldc = N; g.ldres = N; g.alpha = 0.5f; g.act = act; g.out_f32 = out_f32;
  const int saved = g_gemm_variant;
  g_gemm_variant = variant;
  int r = gemm(nullptr, dtype, g);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  if (r == OK) {
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && r == OK; ++i) r = gemm(nullptr, dtype, g);
    (void)hipEventRecord(e1, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) { set_error("gemm bench kernel failed"); r = E_HIP; }
  }
  float ms = 0.f;
  if (r == OK) (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (ms_out) *ms_out = iters > 0 ? ms / iters : 0.0;
  if (r == OK && max_abs_diff) {
    g_gemm_variant = 1;
    g.C = dC1.p;
    r = gemm(nullptr, dtype, g);
    if (r == OK && hipDeviceSynchronize() != hipSuccess) r = E_HIP;
    if (r == OK) {
      const int rows = M < 512 ? M : 512;
      std::vector<float> a((size_t)rows * N), b((size_t)rows * N);
      double md = 0.0;
      for (int part = 0; part < 2 && r == OK; ++part) {
        const size_t off = part == 0 ? 0 : (size_t)(M - rows) * N;
        Dev va, vb;   // views
        va.p = (char*)dC.p + off * (f32out ? 4 : 2); vb.p = (char*)dC1.p + off * (f32out ? 4 : 2);
        r = down_T(va, dtype, f32out, a.data(), a.size());
        if (r == OK) r = down_T(vb, dtype, f32out, b.data(), b.size());
        va.p = nullptr; vb.p = nullptr;
        for (size_t i = 0; i < a.size(); ++i) { const double d = fabs((double)a[i] - (double)b[i]); if (d > md || d != d) md = d; }
      }
      *max_abs_diff = md;
    }
  }
  g_gemm_variant = saved;
  return r;
}

// ---------------------------------------------------------------------------------------------- diarization kernels (diar.hip, resnet.hip)
// Each hook launches exactly the launcher the engine calls, on host floats (rounded to bf16 here when dtype == 1); the form a
// launcher picks follows its lab switch (RVD_SINC_MFMA, RVD_POOLNORM_VEC) as in the engine.

// window_stats: wave [n]; stats [nwin][2] = (mean, 1 / sqrt(var + eps)) of wave[(first + w) step .. + len)
extern "C" int rvb_test_window_stats(const float* wave, int64_t n, int64_t first, int nwin, int64_t step, int len, float eps, float* stats) {
  if (!wave || !stats || n < 1 || first < 0 || nwin < 1 || step < 1 || len < 1 || (first + nwin - 1) * step + len > n) {
    set_error("rvb_test_window_stats: bad argument"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  Dev dw, ds;
  RVB_TRY(up_T(dw, DT_F32, wave, (size_t)n));
  RVB_TRY(ds.alloc((size_t)nwin * 2 * 4));
  RVB_TRY(window_stats(nullptr, (const float*)dw.p, first, nwin, step, len, eps, (float*)ds.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(ds, DT_F32, true, stats, (size_t)nwin * 2);
}

// sinc_conv: out [n_frames][nf] (dtype) = sum_k wave[t stride + k] filt[f][k]; the launcher refuses what neither form covers
extern "C" int rvb_test_sinc_conv(int dtype, const float* wave, int64_t n_samples, const float* filt, int nf, int ksize, int stride,
                                  int64_t n_frames, float* out) {
  if (!wave || !filt || !out || nf < 1 || ksize < 1 || stride < 1 || n_frames < 1 || (n_frames - 1) * stride + ksize > n_samples ||
      (dtype != DT_F32 && dtype != DT_BF16)) {
    set_error("rvb_test_sinc_conv: bad argument"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  Dev dw, df, dout;
  RVB_TRY(up_T(dw, DT_F32, wave, (size_t)n_samples));
  RVB_TRY(up_T(df, DT_F32, filt, (size_t)nf * ksize));
  RVB_TRY(dout.alloc((size_t)n_frames * nf * dt_size(dtype)));
  RVB_TRY(sinc_conv(nullptr, dtype, (const float*)dw.p, (const float*)df.p, dout.p, n_frames, nf, ksize, stride));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, false, out, (size_t)n_frames * nf);
}

// pool_norm on the fields of PoolNormArgs.  Later block: x [W rows_in][ld_in].  First block: craw [craw_rows][C], stats [W][2],
// fsum [C], wn_gamma / wn_beta.  out [W (frames_in / 3)][ld_out], pad columns included.
extern "C" int rvb_test_pool_norm(int dtype, int first_block, const float* x, int rows_in, int ld_in, int frames_in, int C, int ld_out,
                                  const float* gamma, const float* beta, float eps, int W, const float* craw, int64_t craw_rows,
                                  int64_t craw_frame0, int craw_frames_per_step, const float* stats, const float* fsum, float wn_gamma,
                                  float wn_beta, float* out) {
  const int TP = frames_in / 3;
  bool ok = gamma && beta && out && W >= 1 && TP >= 1 && C >= 1 && ld_out >= C && (dtype == DT_F32 || dtype == DT_BF16);
  if (first_block) ok = ok && craw && stats && fsum && craw_frame0 >= 0 && craw_frames_per_step >= 0 &&
                        craw_frame0 + (int64_t)(W - 1) * craw_frames_per_step + 3 * TP <= craw_rows;
  else ok = ok && x && rows_in >= frames_in && ld_in >= C;
  if (!ok) { set_error("rvb_test_pool_norm: bad argument"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dx, dcr, dst, dfs, dg, db, dout;
  PoolNormArgs a{};
  if (first_block) {
    RVB_TRY(up_T(dcr, dtype, craw, (size_t)craw_rows * C));
    RVB_TRY(up_T(dst, DT_F32, stats, (size_t)W * 2));
    RVB_TRY(up_T(dfs, DT_F32, fsum, (size_t)C));
    a.craw = dcr.p; a.craw_frame0 = craw_frame0; a.craw_frames_per_step = craw_frames_per_step;
    a.stats = (const float*)dst.p; a.fsum = (const float*)dfs.p; a.wn_gamma = wn_gamma; a.wn_beta = wn_beta;
  } else {
    RVB_TRY(up_T(dx, dtype, x, (size_t)W * rows_in * ld_in));
    a.x = dx.p; a.rows_in = rows_in; a.ld_in = ld_in;
  }
  RVB_TRY(up_T(dg, DT_F32, gamma, (size_t)C));
  RVB_TRY(up_T(db, DT_F32, beta, (size_t)C));
  const size_t no = (size_t)W * TP * ld_out;
  RVB_TRY(dout.alloc(no * dt_size(dtype)));
  RVB_HIP_CHECK(hipMemset(dout.p, 0x7f, no * dt_size(dtype)));      // unwritten pad columns show up as 3.4e38 / 3.3e38
  a.frames_in = frames_in; a.C = C; a.ld_out = ld_out; a.gamma = (const float*)dg.p; a.beta = (const float*)db.p; a.eps = eps;
  a.out = dout.p; a.W = W;
  RVB_TRY(pool_norm(nullptr, dtype, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, false, out, no);
}

// conv1d5 (bf16): A [rows][cin] with rows >= M + 4, W [60][cin_real][5] as torch stores Conv1d weights (cin_real = 80 for cin 80,
// 60 for cin 64), bias [60]; out [M][64] (filters 60 .. 63 are the zero pads).  The weights are packed as pack_conv1d packs them
// (diar_engine.hip: [64][5][cin]); the device input has M + 8 rows as the engine's, rows M + 4 .. M + 7 hold 1e30 (nobody reads them).
extern "C" int rvb_test_conv1d5(int cin, const float* A, int64_t rows, const float* W, const float* bias, float* out, int64_t M) {
  if (!A || !W || !bias || !out || (cin != 80 && cin != 64) || M < 1 || rows < M + 4) { set_error("rvb_test_conv1d5: bad argument"); return E_ARG; }
  RVB_TRY(need_gpu());
  const int cr = cin == 80 ? 80 : 60, NO = 60, NP = 64, K = 5;
  std::vector<float> pw((size_t)NP * K * cin, 0.f), pb(NP, 0.f);
  for (int o = 0; o < NO; ++o) {
    pb[o] = bias[o];
    for (int c = 0; c < cr; ++c)
      for (int k = 0; k < K; ++k) pw[((size_t)o * K + k) * cin + c] = W[((size_t)o * cr + c) * K + k];
  }
  std::vector<bf16_t> ab((size_t)(M + 8) * cin, f32_to_bf16(1e30f));
  for (size_t i = 0; i < (size_t)(M + 4) * cin; ++i) ab[i] = f32_to_bf16(A[i]);
  Dev da, dw, db, dout;
  RVB_TRY(up_raw(da, ab.data(), ab.size() * 2));
  RVB_TRY(up_T(dw, DT_BF16, pw.data(), pw.size()));
  RVB_TRY(up_T(db, DT_F32, pb.data(), pb.size()));
  RVB_TRY(dout.alloc((size_t)M * NP * 2));
  RVB_TRY(conv1d5(nullptr, DT_BF16, da.p, cin, dw.p, (const float*)db.p, dout.p, M));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, DT_BF16, false, out, (size_t)M * NP);
}

// One bidirectional LSTM layer (hidden 128) as segment_impl runs it: x [W T][in] . w_ih^T + b_ih + b_hh on the GEMM into the
// recurrence kernel's column order (lstm_pack_inproj), then lstm_recurrence.  w_ih [2][4H][in], w_hh [2][4H][H], b_ih / b_hh [2][4H]
// (PyTorch layout, forward then reverse); out [W T][2H] = (forward h | reverse h).
extern "C" int rvb_test_lstm_layer(int dtype, const float* x, int W, int T, int in, const float* w_ih, const float* w_hh, const float* b_ih,
                                   const float* b_hh, float* out) {
  constexpr int H = 128;
  if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !out || W < 1 || T < 1 || in < 8 || (in % 8) || (int64_t)W * T > 0x7fffffff / (8 * H) ||
      (dtype != DT_F32 && dtype != DT_BF16)) {
    set_error("rvb_test_lstm_layer: bad argument"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  std::vector<float> wih((size_t)8 * H * in, 0.f), bias((size_t)8 * H, 0.f);
  for (int d = 0; d < 2; ++d)
    lstm_pack_inproj(w_ih + (size_t)d * 4 * H * in, b_ih + (size_t)d * 4 * H, b_hh + (size_t)d * 4 * H, H, in, in,
                     &wih[(size_t)d * 4 * H * in], &bias[(size_t)d * 4 * H]);
  const size_t R = (size_t)W * T;
  Dev dx, dwi, db, dwh, dxp, dout;
  RVB_TRY(up_T(dx, dtype, x, R * in));
  RVB_TRY(up_T(dwi, dtype, wih.data(), wih.size()));
  RVB_TRY(up_T(db, DT_F32, bias.data(), bias.size()));
  RVB_TRY(up_T(dwh, dtype, w_hh, (size_t)8 * H * H));
  RVB_TRY(dxp.alloc(R * 8 * H * dt_size(dtype)));
  RVB_TRY(dout.alloc(R * 2 * H * dt_size(dtype)));
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dx.p; g.W = dwi.p; g.bias = (const float*)db.p; g.C = dxp.p;
  g.M = (int)R; g.N = 8 * H; g.K = in; g.lda = in; g.ldw = in; g.ldc = 8 * H; g.alpha = 1.f; g.act = ACT_NONE;
  RVB_TRY(gemm(nullptr, dtype, g));
  RVB_TRY(lstm_recurrence(nullptr, dtype, dxp.p, dwh.p, dout.p, W, T));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(dout, dtype, false, out, R * 2 * H);
}

// classifier_logsoftmax: x [M][ldx] (dtype), w [C][in], b [C] fp32; logp [M][C]; cls [M] (nullable)
extern "C" int rvb_test_classifier(int dtype, const float* x, int ldx, const float* w, const float* b, float* logp, uint8_t* cls,
                                   int64_t M, int in, int C) {
  if (!x || !w || !b || !logp || M < 1 || C < 1 || in < 1 || ldx < in || (dtype != DT_F32 && dtype != DT_BF16)) {
    set_error("rvb_test_classifier: bad argument"); return E_ARG;
  }
  RVB_TRY(need_gpu());
  Dev dx, dw, db, dl, dc;
  RVB_TRY(up_T(dx, dtype, x, (size_t)M * ldx));
  RVB_TRY(up_T(dw, DT_F32, w, (size_t)C * in));
  RVB_TRY(up_T(db, DT_F32, b, (size_t)C));
  RVB_TRY(dl.alloc((size_t)M * C * 4));
  if (cls) RVB_TRY(dc.alloc((size_t)M));
  RVB_TRY(classifier_logsoftmax(nullptr, dtype, dx.p, ldx, (const float*)dw.p, (const float*)db.p, (float*)dl.p, (uint8_t*)dc.p, M, in, C));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  if (cls) RVB_HIP_CHECK(hipMemcpy(cls, dc.p, (size_t)M, hipMemcpyDeviceToHost));
  return down_T(dl, DT_F32, true, logp, (size_t)M * C);
}

// tstp_pool: x [B][F][TT][C] (unbordered), item_b [n_items] in [0, B), mask [n_items][mask_len]; stats [n_items][2 C F] = (mean | std)
// with feature index c F + f.  Builds the bordered [B][F + 2][TT + 2][C] plane the kernel reads, its border at 1e3 (never read).
extern "C" int rvb_test_tstp(int dtype, const float* x, int B, const int32_t* item_b, const float* mask, int mask_len, int n_items, int F,
                             int TT, int C, float* stats) {
  bool ok = x && item_b && mask && stats && B >= 1 && mask_len >= 1 && n_items >= 1 && F >= 1 && TT >= 1 && C >= 1 &&
            (dtype == DT_F32 || dtype == DT_BF16);
  for (int i = 0; ok && i < n_items; ++i) ok = item_b[i] >= 0 && item_b[i] < B;
  if (!ok) { set_error("rvb_test_tstp: bad argument"); return E_ARG; }
  RVB_TRY(need_gpu());
  const size_t np = (size_t)B * (F + 2) * (TT + 2) * C;
  std::vector<float> xb(np, 1e3f);
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < F; ++f)
      for (int t = 0; t < TT; ++t)
        memcpy(&xb[(((size_t)b * (F + 2) + f + 1) * (TT + 2) + t + 1) * C], &x[(((size_t)b * F + f) * TT + t) * C], (size_t)C * 4);
  Dev dx, di, dm, ds;
  RVB_TRY(up_T(dx, dtype, xb.data(), np));
  RVB_TRY(up_raw(di, item_b, (size_t)n_items * 4));
  RVB_TRY(up_T(dm, DT_F32, mask, (size_t)n_items * mask_len));
  RVB_TRY(ds.alloc((size_t)n_items * 2 * C * F * dt_size(dtype)));
  RVB_TRY(tstp_pool(nullptr, dtype, dx.p, (const int*)di.p, (const float*)dm.p, mask_len, n_items, F, TT, C, ds.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_T(ds, dtype, false, stats, (size_t)n_items * 2 * C * F);
}

// ---------------------------------------------------------------------------------------------- embedding trunk (resnet.hip, conv_*.hip)
namespace {
// unbordered NHWC [B][F][T][C] host floats -> bordered [B][F + 2][T + 2][C] in dtype (zero border) + `slack` zero bytes behind it
int up_bordered(Dev& d, int dtype, const float* src, int B, int F, int T, int C, size_t slack) {
  const size_t n = (size_t)B * (F + 2) * (T + 2) * C, es = dt_size(dtype);
  RVB_TRY(d.alloc(n * es + slack));
  RVB_HIP_CHECK(hipMemset(d.p, 0, n * es + slack));
  std::vector<float> p(n, 0.f);
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < F; ++f)
      for (int t = 0; t < T; ++t)
        memcpy(&p[(((size_t)b * (F + 2) + f + 1) * (T + 2) + t + 1) * C], &src[(((size_t)b * F + f) * T + t) * C], (size_t)C * 4);
  if (dtype == DT_F32) { RVB_HIP_CHECK(hipMemcpy(d.p, p.data(), n * 4, hipMemcpyHostToDevice)); return OK; }
  std::vector<bf16_t> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = f32_to_bf16(p[i]);
  RVB_HIP_CHECK(hipMemcpy(d.p, h.data(), n * 2, hipMemcpyHostToDevice));
  return OK;
}
// bordered device plane (+ slack bytes) -> unbordered host floats; E_STATE if anything outside the interior is not zero
int down_bordered(const Dev& d, int dtype, float* dst, int B, int F, int T, int C, size_t slack, const char* who) {
  const size_t n = (size_t)B * (F + 2) * (T + 2) * C, es = dt_size(dtype);
  std::vector<unsigned char> raw(n * es + slack);
  RVB_HIP_CHECK(hipMemcpy(raw.data(), d.p, raw.size(), hipMemcpyDeviceToHost));
  for (size_t i = n * es; i < raw.size(); ++i)
    if (raw[i]) { set_error(std::string(who) + ": the kernel wrote past the end of its output plane"); return E_STATE; }
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < F + 2; ++f)
      for (int t = 0; t < T + 2; ++t) {
        const size_t at = (((size_t)b * (F + 2) + f) * (T + 2) + t) * C;
        const bool border = f == 0 || f == F + 1 || t == 0 || t == T + 1;
        for (int c = 0; c < C; ++c) {
          float v;
          if (dtype == DT_F32) memcpy(&v, &raw[(at + c) * 4], 4);
          else { bf16_t h; memcpy(&h, &raw[(at + c) * 2], 2); v = bf16_to_f32(h); }
          if (border) {
            bool zero = true;
            for (size_t k = 0; k < es; ++k) zero = zero && raw[(at + c) * es + k] == 0;
            if (!zero) { set_error(std::string(who) + ": the kernel wrote into the zero border"); return E_STATE; }
          } else {
            dst[(((size_t)b * F + f - 1) * T + t - 1) * C + c] = v;
          }
        }
      }
  return OK;
}
constexpr size_t kSlack = 64 * 1024;      // zeros behind every device tensor of the conv hooks (kernels that read a row ahead stay inside)
}  // namespace

// One convolution of the trunk through a named path, on host floats.  x [B][Fi][Ti][Cin] (unbordered NHWC), w [Cout][Cin][k][k] as torch
// stores it (BatchNorm folded; k = 3 for taps 9, 1 for taps 1), bias [Cout], res [B][Fo][To][Cout] or null; out [B][Fo][To][Cout],
// Fo = (Fi - 1) / stride + 1 (the same for To).  Fused projection shortcut (x2 non-null): x2 [B][Fi2][Ti2][Cin2], w2 [Cout][Cin2],
// stride2, with Fo = (Fi2 - 1) / stride2 + 1 (To alike); bias is then the sum of both biases and res must be null (pack_fused_shortcut).
// path: 0 = conv2d()'s own dispatch, with w_ig present when the engine would pack it for this shape (conv_igemm_packed);
// 1 = resnet.hip's direct kernel; 2 = conv_gemm.hip's implicit GEMM; 3 = conv_row64.hip; 4 = conv_stream.hip.  A path that does not
// apply to the shape (lab switches included) is refused with E_STATE before anything runs.  ran[2] = {kernel that ran, 1 .. 4 as
// `path`; its tile: output channels per workgroup (direct), pixels per tile (implicit GEMM: 256 | 512 wide), 0 (row64), workgroups
// per row of tiles (stream)}.  The output plane is zero-filled first; E_STATE if the kernel wrote into its border or past its end.
extern "C" int rvb_test_conv2d(int dtype, int path, const float* x, const float* w, const float* bias, const float* res, float* out,
                               int B, int Fi, int Ti, int Cin, int Cout, int stride, int taps, int relu, const float* x2,
                               const float* w2, int Fi2, int Ti2, int Cin2, int stride2, int32_t* ran) {
  const int ck = dtype == DT_BF16 ? 32 : 16;
  bool ok = x && w && bias && out && ran && (dtype == DT_F32 || dtype == DT_BF16) && path >= 0 && path <= 4 && B >= 1 && Fi >= 1 &&
            Ti >= 1 && Cin >= 1 && Cout >= 1 && Cin % ck == 0 && Cout % 32 == 0 && (stride == 1 || stride == 2) && (taps == 9 || taps == 1);
  const int Fo = ok ? (Fi - 1) / stride + 1 : 0, To = ok ? (Ti - 1) / stride + 1 : 0;
  ok = ok && (int64_t)(Fi + 2) * (Ti + 2) * Cin < ((int64_t)1 << 30) && (int64_t)(Fo + 2) * (To + 2) * Cout < ((int64_t)1 << 30) &&
       (int64_t)B * (Fi + 2) * (Ti + 2) * Cin < ((int64_t)1 << 31) && (int64_t)B * (Fo + 2) * (To + 2) * Cout < ((int64_t)1 << 31);
  if (x2)
    ok = ok && w2 && !res && (stride2 == 1 || stride2 == 2) && Fi2 >= 1 && Ti2 >= 1 && Cin2 >= 1 && Cin2 % ck == 0 &&
         Fo == (Fi2 - 1) / stride2 + 1 && To == (Ti2 - 1) / stride2 + 1 && (int64_t)B * (Fi2 + 2) * (Ti2 + 2) * Cin2 < ((int64_t)1 << 31);
  if (!ok) { set_error("rvb_test_conv2d: bad argument"); return E_ARG; }
  // which kernel runs: decided on the shape alone (the host pointers stand in for the device tensors they will become)
  const int k = taps == 9 ? 3 : 1;
  const bool pack_ig = path == 2 || (path == 0 && conv_igemm_packed(dtype, k, stride, Cin, Cout));
  ConvArgs a{};
  a.in = x; a.w = w; a.bias = bias; a.res = res; a.out = out;
  a.B = B; a.Fi = Fi; a.Ti = Ti; a.Cin = Cin; a.Fo = Fo; a.To = To; a.Cout = Cout; a.stride = stride; a.taps = taps; a.relu = relu;
  a.w_ig = pack_ig ? w : nullptr;
  if (x2) { a.in2 = x2; a.Cin2 = Cin2; a.Fi2 = Fi2; a.Ti2 = Ti2; a.stride2 = stride2; }
  int kind = 0;
  if (path == 0) kind = conv_igemm_applicable(dtype, a) ? 2 : x2 ? 0 : conv_row64_applicable(dtype, a) ? 3 : conv_stream_applicable(dtype, a) ? 4 : 1;
  else if (path == 1) kind = x2 ? 0 : 1;
  else if (path == 2) kind = conv_igemm_applicable(dtype, a) ? 2 : 0;
  else if (path == 3) kind = !x2 && conv_row64_applicable(dtype, a) ? 3 : 0;
  else kind = !x2 && conv_stream_applicable(dtype, a) ? 4 : 0;
  if (kind == 0) { set_error("rvb_test_conv2d: the path does not apply to this shape (or is switched off)"); return E_STATE; }
  RVB_TRY(need_gpu());
  Dev dx, dw, dwg, db, dr, dout, dx2;
  RVB_TRY(up_bordered(dx, dtype, x, B, Fi, Ti, Cin, kSlack));
  if (res) RVB_TRY(up_bordered(dr, dtype, res, B, Fo, To, Cout, kSlack));
  if (x2) RVB_TRY(up_bordered(dx2, dtype, x2, B, Fi2, Ti2, Cin2, kSlack));
  std::vector<float> pw((size_t)taps * Cin * Cout);
  conv_pack_direct(w, nullptr, Cout, Cin, taps, ck, pw.data());
  RVB_TRY(up_T(dw, dtype, pw.data(), pw.size()));
  if (kind == 2) {
    std::vector<float> pg((size_t)Cout * ((size_t)taps * Cin + (x2 ? Cin2 : 0)));
    if (x2) conv_pack_fused_shortcut(w, nullptr, w2, nullptr, Cout, Cin, Cin2, pg.data());
    else conv_pack_igemm(w, nullptr, Cout, Cin, taps, (size_t)taps * Cin, pg.data());
    RVB_TRY(up_T(dwg, DT_BF16, pg.data(), pg.size()));
  }
  RVB_TRY(up_raw(db, bias, (size_t)Cout * 4));
  const size_t no = (size_t)B * (Fo + 2) * (To + 2) * Cout * dt_size(dtype);
  RVB_TRY(dout.alloc(no + kSlack));
  RVB_HIP_CHECK(hipMemset(dout.p, 0, no + kSlack));
  a.in = dx.p; a.w = dw.p; a.bias = (const float*)db.p; a.res = dr.p; a.out = dout.p; a.w_ig = kind == 2 ? dwg.p : nullptr;
  a.in2 = dx2.p;
  ran[0] = kind;
  ran[1] = kind == 1 ? conv2d_direct_nt(a) : kind == 2 ? (conv_igemm_wide(a) ? 512 : 256) : kind == 4 ? conv_stream_split(a) : 0;
  if (path == 0) RVB_TRY(conv2d(nullptr, dtype, a));
  else if (kind == 1) RVB_TRY(conv2d_direct(nullptr, dtype, a));
  else if (kind == 2) RVB_TRY(conv_igemm(nullptr, a));
  else if (kind == 3) RVB_TRY(conv_row64(nullptr, a));
  else RVB_TRY(conv_stream(nullptr, a));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  return down_bordered(dout, dtype, out, B, Fo, To, Cout, kSlack, "rvb_test_conv2d");
}

// The stem of the trunk as run_trunk runs it: emb_window_mean over ALL n_windows windows of the fbank rows fb [n_rows][80] (window w
// = rows w frames_per_step .. + nfr), then emb_conv1 on the windows win [B] (any order, repeats allowed) with w [C][1][3][3] (BatchNorm
// folded), bias [C].  mean [n_windows][80] (fp32); out [B][F][nfr][C] (unbordered; the bordered plane's border must stay zero).
extern "C" int rvb_test_emb_stem(int dtype, const float* fb, int64_t n_rows, const int64_t* win, int B, int n_windows, int frames_per_step,
                                 int nfr, int F, int C, const float* w, const float* bias, float* mean, float* out) {
  bool ok = fb && win && w && bias && mean && out && (dtype == DT_F32 || dtype == DT_BF16) && B >= 1 && n_windows >= 1 &&
            frames_per_step >= 1 && nfr >= 1 && F >= 1 && F <= 80 && (C == 8 || C == 16 || C == 32) &&
            (int64_t)(n_windows - 1) * frames_per_step + nfr <= n_rows && (int64_t)B * (F + 2) * (nfr + 2) * C < ((int64_t)1 << 31);
  for (int b = 0; ok && b < B; ++b) ok = win[b] >= 0 && win[b] < n_windows && win[b] * frames_per_step + nfr <= n_rows;
  if (!ok) { set_error("rvb_test_emb_stem: bad argument"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dfb, dwin, dmean, dw, db, dout;
  RVB_TRY(up_raw(dfb, fb, (size_t)n_rows * 80 * 4));
  RVB_TRY(up_raw(dwin, win, (size_t)B * 8));
  RVB_TRY(dmean.alloc((size_t)n_windows * 80 * 4));
  RVB_TRY(up_raw(dw, w, (size_t)C * 9 * 4));
  RVB_TRY(up_raw(db, bias, (size_t)C * 4));
  const size_t no = (size_t)B * (F + 2) * (nfr + 2) * C * dt_size(dtype);
  RVB_TRY(dout.alloc(no + kSlack));
  RVB_HIP_CHECK(hipMemset(dout.p, 0, no + kSlack));
  RVB_TRY(emb_window_mean(nullptr, (const float*)dfb.p, nullptr, n_windows, frames_per_step, nfr, (float*)dmean.p));
  RVB_TRY(emb_conv1(nullptr, dtype, (const float*)dfb.p, (const int64_t*)dwin.p, (const float*)dmean.p, (const float*)dw.p, (const float*)db.p,
                  dout.p, B, F, nfr, frames_per_step, C));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(mean, dmean.p, (size_t)n_windows * 80 * 4, hipMemcpyDeviceToHost));
  return down_bordered(dout, dtype, out, B, F, nfr, C, kSlack, "rvb_test_emb_stem");
}

// ---------------------------------------------------------------------------------------------- clustering (linkage.hip)
// pdist + nn_init as centroid_linkage() launches them: X [n][d] fp64 -> D [n][n], neighbor [n], min_dist [n].  The three device
// outputs start as all-ones bytes (NaN / -1) and come back whole, so an element no kernel wrote comes back as that (slot n - 1 of
// neighbor and min_dist always does: nn_init's grid is n - 1).
extern "C" int rvb_test_pdist_nn(const double* X, int n, int d, double* D, int32_t* neighbor, double* min_dist) {
  if (!X || !D || !neighbor || !min_dist || n < 2 || d < 1 || n > 46000) { set_error("rvb_test_pdist_nn: bad argument"); return E_ARG; }
  RVB_TRY(need_gpu());
  Dev dX, dD, dN, dM;
  RVB_TRY(up_raw(dX, X, (size_t)n * d * 8));
  RVB_TRY(dD.alloc((size_t)n * n * 8));
  RVB_TRY(dN.alloc((size_t)n * 4));
  RVB_TRY(dM.alloc((size_t)n * 8));
  RVB_HIP_CHECK(hipMemset(dD.p, 0xff, (size_t)n * n * 8));
  RVB_HIP_CHECK(hipMemset(dN.p, 0xff, (size_t)n * 4));
  RVB_HIP_CHECK(hipMemset(dM.p, 0xff, (size_t)n * 8));
  RVB_TRY(pdist(nullptr, (const double*)dX.p, n, d, (double*)dD.p));
  RVB_TRY(nn_init(nullptr, (const double*)dD.p, n, (int*)dN.p, (double*)dM.p));
  RVB_HIP_CHECK(hipDeviceSynchronize());
  RVB_HIP_CHECK(hipMemcpy(D, dD.p, (size_t)n * n * 8, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(neighbor, dN.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(min_dist, dM.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return OK;
}

// centroid_linkage() without an engine: the allocations, the initial state and the 4096-byte control block of rvd_centroid_linkage
// (diar_engine.hip), the status check and the slot-to-id conversion; `workgroups` as rvd_set_linkage_workgroups takes it.  ran [4] =
// what centroid_linkage() reports (kernels.h); retries (nullable) = the merge loop's count of stale candidates it re-evaluated.  Z is
// written only when the call succeeds.  The RVD_LINKAGE_* switches apply (this library reads them).
extern "C" int rvb_test_centroid_linkage(const double* X, int n, int d, int workgroups, double* Z, int32_t* ran, double* retries) {
  if (!X || !Z || !ran || n < 1 || d < 1) { set_error("rvb_test_centroid_linkage: bad argument"); return E_ARG; }
  if (n > 46000) { set_error("rvb_test_centroid_linkage: more than 46000 points"); return E_UNSUPPORTED; }
  if (!(workgroups == 0 || workgroups == 1 || workgroups == 2 || workgroups == 4 || workgroups == 8 || workgroups == 16)) {
    set_error("rvb_test_centroid_linkage: workgroups: 0 (default), 1, 2, 4, 8 or 16");
    return E_ARG;
  }
  ran[0] = ran[1] = ran[2] = ran[3] = 0;
  if (retries) *retries = 0.0;
  if (n == 1) return OK;
  RVB_TRY(need_gpu());
  Dev dX, dD, dI, dM, dZ, dC;
  RVB_TRY(dC.alloc(4096));
  RVB_TRY(up_raw(dX, X, (size_t)n * d * 8));
  RVB_TRY(dD.alloc((size_t)n * n * 8));
  std::vector<int> init((size_t)3 * n);     // [cluster_id | neighbor | size as uint16]
  for (int i = 0; i < n; ++i) { init[i] = i; init[n + i] = -1; ((uint16_t*)&init[2 * (size_t)n])[i] = 1; }
  std::vector<double> inf(n, INFINITY);
  RVB_TRY(up_raw(dI, init.data(), init.size() * 4));
  RVB_TRY(up_raw(dM, inf.data(), (size_t)n * 8));
  RVB_TRY(dZ.alloc((size_t)(n - 1) * 4 * 8));
  int r4[4] = {0, 0, 0, 0};
  const int rc = centroid_linkage(nullptr, (const double*)dX.p, n, d, (double*)dD.p, (uint16_t*)((int*)dI.p + 2 * n), (int*)dI.p,
                                  (int*)dI.p + n, (double*)dM.p, (double*)dZ.p, dC.p, workgroups, r4);
  for (int i = 0; i < 4; ++i) ran[i] = r4[i];
  if (rc != OK) { (void)hipDeviceSynchronize(); return rc; }
  RVB_HIP_CHECK(hipDeviceSynchronize());
  double status = 0.0;
  RVB_HIP_CHECK(hipMemcpy(&status, (double*)dM.p + (n - 1), 8, hipMemcpyDeviceToHost));
  if (status < 0.0) { set_error("rvb_test_centroid_linkage: the merge loop found no candidate pair (non-finite embeddings?)"); return E_ARG; }
  if (retries) *retries = status;
  RVB_HIP_CHECK(hipMemcpy(Z, dZ.p, (size_t)(n - 1) * 4 * 8, hipMemcpyDeviceToHost));
  linkage_slots_to_ids(Z, n);
  return OK;
}

// centroid_linkage_many() without an engine, then -- as rvd_centroid_linkage_many does -- the single call (the hook above, default
// workgroups) on every problem it routed away.  route [n_problems]: 1 / 2 = the batched loop that ran, 0 = the single call,
// -1 = fewer than 2 points.  Z as rvd_centroid_linkage_many lays it out; on failure its contents are unspecified.
extern "C" int rvb_test_centroid_linkage_many(const double* X, const int32_t* n, int n_problems, int d, double* Z, int32_t* route) {
  if (!n || !route || n_problems < 1 || d < 1) { set_error("rvb_test_centroid_linkage_many: bad argument"); return E_ARG; }
  int64_t points = 0, rows = 0;
  for (int p = 0; p < n_problems; ++p) {
    if (n[p] < 0 || n[p] > 46000) { set_error("rvb_test_centroid_linkage_many: problem " + std::to_string(p) + ": size outside 0 .. 46000"); return E_ARG; }
    points += n[p]; rows += n[p] > 1 ? n[p] - 1 : 0;
  }
  if ((points > 0 && !X) || (rows > 0 && !Z)) { set_error("rvb_test_centroid_linkage_many: null X or Z"); return E_ARG; }
  for (int p = 0; p < n_problems; ++p) route[p] = -1;
  if (rows == 0) return OK;
  RVB_TRY(need_gpu());
  RVB_TRY(centroid_linkage_many(nullptr, X, n, n_problems, d, Z, route, nullptr));
  int64_t ox = 0, oz = 0;
  for (int p = 0; p < n_problems; ++p) {
    if (route[p] == 0) {
      int32_t ran[4];
      const int rc = rvb_test_centroid_linkage(X + ox * d, n[p], d, 0, Z + oz * 4, ran, nullptr);
      if (rc != OK) { set_error("rvb_test_centroid_linkage_many: problem " + std::to_string(p) + ": " + rvb::last_error()); return rc; }
    }
    ox += n[p]; oz += n[p] > 1 ? n[p] - 1 : 0;
  }
  return OK;
}

// ---- hooks into the engine's host code (engine_impl.h, trie.h)
// host only: the rescoring trie of given hypotheses (tests/test_search_native.py checks it against a Python trie).
// tokens: the hypotheses back to back; lens / chunk_of: per hypothesis (chunk ids ascending).  Outputs sized by the caller:
// rows <= P = sum(len + 1); tok, pos [rows]; path, tgt, pair_slot [P]; hq_start, hq_len, hq_pos0 [n_hyps]; tgt_ptr [rows + 1].
extern "C" int rvb_test_build_trie(const int32_t* tokens, const int32_t* lens, const int32_t* chunk_of, int n_hyps, int n_chunks, int sos,
                                   int eos, int reversed, int32_t* n_rows, int32_t* tok, int32_t* pos, int32_t* path, int32_t* hq_start,
                                   int32_t* hq_len, int32_t* hq_pos0, int32_t* tgt_ptr, int32_t* tgt, int32_t* pair_slot, int32_t* n_work) {
  if (!tokens || !lens || !chunk_of || !n_rows || n_hyps < 0) { set_error("rvb_test_build_trie: bad argument"); return E_ARG; }
  std::vector<HypRef> hyps;
  std::vector<int> first(n_hyps);
  int P = 0, off = 0;
  for (int i = 0; i < n_hyps; ++i) { hyps.push_back({chunk_of[i], i, lens[i], P}); first[i] = off; P += lens[i] + 1; off += lens[i]; }
  TrieBatch t;
  auto seq = [&](const HypRef& h, int j) { return tokens[first[h.idx] + (reversed ? h.len - 1 - j : j)]; };
  build_trie_range(hyps.data(), hyps.data() + hyps.size(), 0, n_chunks, sos, eos, seq, &t);
  {   // the engine builds the same trie chunk by chunk and stitches the parts (merge_tries): both forms must agree exactly
    std::vector<TrieBatch> part(std::max(n_chunks, 0));
    size_t a = 0;
    for (int b = 0; b < n_chunks; ++b) {
      size_t z = a;
      while (z < hyps.size() && hyps[z].chunk == b) ++z;
      build_trie_range(hyps.data() + a, hyps.data() + z, b, 1, sos, eos, seq, &part[b]);
      a = z;
    }
    TrieBatch m;
    merge_tries(part, &m);
    const bool same = m.R == t.R && m.P == t.P && m.max_chunk_rows == t.max_chunk_rows && m.tok == t.tok && m.pos == t.pos &&
                      m.path == t.path && m.hq_start == t.hq_start && m.hq_len == t.hq_len && m.hq_pos0 == t.hq_pos0 &&
                      m.hkv_start == t.hkv_start && m.hkv_len == t.hkv_len && m.crow_start == t.crow_start &&
                      m.crow_len == t.crow_len && m.tgt_ptr == t.tgt_ptr && m.tgt == t.tgt && m.pair_slot == t.pair_slot &&
                      m.work == t.work;
    if (a != hyps.size() || !same) {
      std::string which;
#define RVB_DIFF(f) if (!(m.f == t.f)) which += std::string(" ") + #f;
      RVB_DIFF(R) RVB_DIFF(P) RVB_DIFF(max_chunk_rows) RVB_DIFF(tok) RVB_DIFF(pos) RVB_DIFF(path) RVB_DIFF(hq_start) RVB_DIFF(hq_len)
      RVB_DIFF(hq_pos0) RVB_DIFF(hkv_start) RVB_DIFF(hkv_len) RVB_DIFF(crow_start) RVB_DIFF(crow_len) RVB_DIFF(tgt_ptr) RVB_DIFF(tgt)
      RVB_DIFF(pair_slot) RVB_DIFF(work)
#undef RVB_DIFF
      set_error("rvb_test_build_trie: the stitched per-chunk tries differ from the batch trie in:" + which);
      return E_STATE;
    }
  }
  *n_rows = t.R;
  if (n_work) *n_work = (int32_t)t.work.size() / 2;
  auto cp = [](int32_t* dst, const std::vector<int32_t>& v) { if (dst) memcpy(dst, v.data(), v.size() * 4); };
  cp(tok, t.tok); cp(pos, t.pos); cp(path, t.path); cp(hq_start, t.hq_start); cp(hq_len, t.hq_len); cp(hq_pos0, t.hq_pos0);
  cp(tgt_ptr, t.tgt_ptr); cp(tgt, t.tgt); cp(pair_slot, t.pair_slot);
  return OK;
}

// host only: HostPool runs `rounds` jobs of `n_threads` threads each; every job hands out `items` work items through an atomic
// counter (the pattern of the CTC search) and the call checks that each item was executed exactly once in every round.
extern "C" int rvb_test_host_pool(int n_threads, int items, int rounds) {
  if (n_threads < 1 || items < 0 || rounds < 1) { set_error("rvb_test_host_pool: bad argument"); return E_ARG; }
  HostPool pool;
  std::vector<std::atomic<int>> hits(items);
  for (int r = 0; r < rounds; ++r) {
    for (auto& h : hits) h.store(0);
    std::atomic<int> next(0), entered(0);
    const unsigned n = (unsigned)std::max(1, n_threads - (r % 3));     // the pool grows and is reused with fewer threads
    pool.run(n, [&] {
      entered.fetch_add(1);
      for (int i = next.fetch_add(1); i < items; i = next.fetch_add(1)) hits[i].fetch_add(1);
    });
    if (entered.load() != (int)n) { set_error("rvb_test_host_pool: a job was not run by the requested number of threads"); return E_STATE; }
    for (int i = 0; i < items; ++i)
      if (hits[i].load() != 1) { set_error("rvb_test_host_pool: work item executed " + std::to_string(hits[i].load()) + " times"); return E_STATE; }
  }
  return OK;
}

extern "C" int rvb_test_fbank_ex(const int16_t* pcm, const float* wave, int64_t n_samples, float* feats) {
  if ((pcm == nullptr) == (wave == nullptr) || !feats || n_samples < 0) { set_error("rvb_test_fbank_ex: one of pcm / wave, feats and n_samples >= 0 are needed"); return E_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: librvb has no CPU fallback"); return E_HIP; }
  rvb_engine e;   // default stream, only the fbank tables are used
  RVB_TRY(make_fbank_tables(&e));
  const int64_t nf = rvb_num_frames(n_samples);
  const size_t in_bytes = (size_t)n_samples * (pcm ? 2 : 4), out_bytes = (size_t)(nf + 4) * 80 * 4;
  void* din = nullptr;     // not a DevBuf: exactly the waveform's bytes, so that a read past its end is a read past the allocation
  DevBuf df;
  int r = df.ensure(out_bytes);
  if (r == OK && in_bytes && hipMalloc(&din, in_bytes) != hipSuccess) { set_error("rvb_test_fbank_ex: hipMalloc failed"); r = E_NOMEM; }
  if (r == OK && in_bytes && hipMemcpy(din, pcm ? (const void*)pcm : (const void*)wave, in_bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("rvb_test_fbank_ex: upload failed"); r = E_HIP; }
  if (r == OK && hipMemset(df.p, 0xff, out_bytes) != hipSuccess) { set_error("rvb_test_fbank_ex: memset failed"); r = E_HIP; }
  FbankTables t{e.fb_window.as<float>(), e.fb_twiddle.as<float>(), e.fb_melw.as<float>(), e.fb_lo.as<int>(), e.fb_hi.as<int>()};
  if (r == OK) r = pcm ? fbank(nullptr, (const int16_t*)din, nf, df.as<float>(), t) : fbank_f32(nullptr, (const float*)din, nf, df.as<float>(), t);
  if (r == OK && hipDeviceSynchronize() != hipSuccess) { set_error("fbank kernel failed"); r = E_HIP; }
  if (r == OK && hipMemcpy(feats, df.p, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) { set_error("rvb_test_fbank_ex: download failed"); r = E_HIP; }
  if (din) (void)hipFree(din);
  df.release();
  for (DevBuf* b : {&e.fb_window, &e.fb_twiddle, &e.fb_melw, &e.fb_lo, &e.fb_hi}) b->release();
  return r;
}

extern "C" int rvb_test_fbank_batch(const void* const* data, const int32_t* sample_format, const int64_t* n_samples, const int64_t* offset,
                                    int n_rec, int chunk_size, float* feats) {
  if (!data || !sample_format || !n_samples || !feats || n_rec <= 0 || n_rec > 65536 || chunk_size < 7) { set_error("rvb_test_fbank_batch: bad argument"); return E_ARG; }
  std::vector<int64_t> off(n_rec), nfr(n_rec), first(n_rec + 1), frame0(n_rec + 1);
  std::vector<FbankRec> rec(n_rec);
  int64_t end[2] = {0, 0};               // elements of the int16 / the float buffer
  for (int r = 0; r < n_rec; ++r) {
    if ((sample_format[r] != RVB_SAMPLE_I16 && sample_format[r] != RVB_SAMPLE_F32) || n_samples[r] < 0 || (!data[r] && n_samples[r] > 0)) {
      set_error("rvb_test_fbank_batch: bad recording " + std::to_string(r)); return E_ARG;
    }
    const int k = sample_format[r] == RVB_SAMPLE_F32;
    off[r] = offset ? offset[r] : end[k];
    if (off[r] < end[k]) { set_error("rvb_test_fbank_batch: offsets must not be negative, overlap or go backwards (recording " + std::to_string(r) + ")"); return E_ARG; }
    end[k] = off[r] + n_samples[r];
  }
  RVB_TRY(rvb_batch_plan(n_samples, n_rec, chunk_size, nfr.data(), first.data(), nullptr));
  for (int r = 0; r < n_rec; ++r) {
    frame0[r] = r ? frame0[r - 1] + nfr[r - 1] : 0;
    rec[r] = FbankRec{off[r], first[r] * chunk_size, sample_format[r] == RVB_SAMPLE_F32 ? 1 : 0, 0};
  }
  frame0[n_rec] = frame0[n_rec - 1] + nfr[n_rec - 1];
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: librvb has no CPU fallback"); return E_HIP; }
  rvb_engine e;   // default stream, only the fbank tables are used
  RVB_TRY(make_fbank_tables(&e));
  const int64_t rows = first[n_rec] * chunk_size;
  const size_t out_bytes = (size_t)(rows + 4) * 80 * 4;
  void *d16 = nullptr, *d32 = nullptr, *dfr = nullptr, *drec = nullptr;     // exactly the bytes: a read past the end is a read past the allocation
  DevBuf df;
  int r = df.ensure(out_bytes);
  auto fail = [&](const char* what) { set_error(std::string("rvb_test_fbank_batch: ") + what); return E_HIP; };
  if (r == OK && end[0] && hipMalloc(&d16, (size_t)end[0] * 2) != hipSuccess) r = fail("hipMalloc failed");
  if (r == OK && end[1] && hipMalloc(&d32, (size_t)end[1] * 4) != hipSuccess) r = fail("hipMalloc failed");
  if (r == OK && (hipMalloc(&dfr, frame0.size() * 8) != hipSuccess || hipMalloc(&drec, rec.size() * sizeof(FbankRec)) != hipSuccess)) r = fail("hipMalloc failed");
  for (int i = 0; r == OK && i < n_rec; ++i) {
    if (!n_samples[i]) continue;
    const bool f32 = sample_format[i] == RVB_SAMPLE_F32;
    void* dst = f32 ? (void*)((float*)d32 + off[i]) : (void*)((int16_t*)d16 + off[i]);
    if (hipMemcpy(dst, data[i], (size_t)n_samples[i] * (f32 ? 4 : 2), hipMemcpyHostToDevice) != hipSuccess) r = fail("upload failed");
  }
  if (r == OK && (hipMemcpy(dfr, frame0.data(), frame0.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
                  hipMemcpy(drec, rec.data(), rec.size() * sizeof(FbankRec), hipMemcpyHostToDevice) != hipSuccess)) r = fail("upload failed");
  if (r == OK && hipMemset(df.p, 0xff, out_bytes) != hipSuccess) r = fail("memset failed");
  FbankTables t{e.fb_window.as<float>(), e.fb_twiddle.as<float>(), e.fb_melw.as<float>(), e.fb_lo.as<int>(), e.fb_hi.as<int>()};
  if (r == OK) r = fbank_batch(nullptr, (const int16_t*)d16, (const float*)d32, (const int64_t*)dfr, (const FbankRec*)drec, n_rec, frame0[n_rec],
                               df.as<float>(), rows, t);
  if (r == OK && hipDeviceSynchronize() != hipSuccess) r = fail("fbank_batch kernel failed");
  if (r == OK && hipMemcpy(feats, df.p, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) r = fail("download failed");
  for (void* q : {d16, d32, dfr, drec}) if (q) (void)hipFree(q);
  df.release();
  for (DevBuf* b : {&e.fb_window, &e.fb_twiddle, &e.fb_melw, &e.fb_lo, &e.fb_hi}) b->release();
  return r;
}

extern "C" int rvb_test_fbank(const int16_t* pcm, int64_t n_samples, float* feats) {
  if (!pcm || !feats || n_samples < 0) { set_error("rvb_test_fbank: null argument"); return E_ARG; }
  const int64_t nf = rvb_num_frames(n_samples);
  std::vector<float> all((size_t)(nf + 4) * 80);
  RVB_TRY(rvb_test_fbank_ex(pcm, nullptr, n_samples, all.data()));
  memcpy(feats, all.data(), (size_t)nf * 80 * 4);
  return OK;
}

// ---- pause_chunks.hip
#include "pause_chunks.h"

namespace {
struct HipMem {      // a device allocation of exactly the bytes asked for, freed on every way out
  void* p = nullptr;
  ~HipMem() { if (p) (void)hipFree(p); }
  int alloc(const char* who, size_t bytes) {
    if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) { p = nullptr; (void)hipGetLastError(); set_error(std::string(who) + ": hipMalloc of " + std::to_string(bytes) + " bytes failed"); return E_NOMEM; }
    return OK;
  }
};
int need_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error(std::string(who) + ": no HIP device available: librvb has no CPU fallback"); return E_HIP; }
  return OK;
}
}  // namespace

extern "C" int rvb_test_pause_cuts(const float* feats, int64_t n_rows, const int64_t* row0, const int64_t* n_frames, int n_rec, int chunk_size,
                                   int search, int h, int32_t* starts, int64_t capacity, int32_t* counts) {
  const char* who = "rvb_test_pause_cuts";
  RVB_TRY(pause_check_args(who, chunk_size, search, h));
  if (!feats || !row0 || !n_frames || !starts || !counts || n_rows < 1 || n_rec < 1 || n_rec > 65536 || capacity < 0) { set_error(std::string(who) + ": bad argument"); return E_ARG; }
  std::vector<PauseRec> rec(n_rec);
  std::vector<int64_t> frame0(n_rec + 1, 0);
  int64_t tab = 0;
  for (int r = 0; r < n_rec; ++r) {
    if (row0[r] < 0 || n_frames[r] < 0 || n_frames[r] > (1 << 30) || row0[r] + n_frames[r] > n_rows) {
      set_error(std::string(who) + ": recording " + std::to_string(r) + " lies outside the " + std::to_string(n_rows) + " rows"); return E_ARG;
    }
    const int64_t cap = pause_max_pieces(n_frames[r], chunk_size, search);
    rec[r] = PauseRec{row0[r], tab, (int32_t)n_frames[r], (int32_t)cap};
    frame0[r + 1] = frame0[r] + n_frames[r];
    tab += cap;
  }
  RVB_TRY(need_device(who));
  HipMem df, dl, dr, d0, dt, dc;
  RVB_TRY(df.alloc(who, (size_t)n_rows * 80 * 4));
  RVB_TRY(dl.alloc(who, (size_t)n_rows * 4));
  RVB_TRY(dr.alloc(who, rec.size() * sizeof(PauseRec)));
  RVB_TRY(d0.alloc(who, frame0.size() * 8));
  RVB_TRY(dt.alloc(who, (size_t)std::max<int64_t>(tab, 1) * 4));
  RVB_TRY(dc.alloc(who, (size_t)n_rec * 4));
  RVB_HIP_CHECK(hipMemcpy(df.p, feats, (size_t)n_rows * 80 * 4, hipMemcpyHostToDevice));
  RVB_HIP_CHECK(hipMemset(dl.p, 0xff, (size_t)n_rows * 4));            // e of a row nobody owns: NaN
  RVB_HIP_CHECK(hipMemcpy(dr.p, rec.data(), rec.size() * sizeof(PauseRec), hipMemcpyHostToDevice));
  RVB_HIP_CHECK(hipMemcpy(d0.p, frame0.data(), frame0.size() * 8, hipMemcpyHostToDevice));
  RVB_TRY(pause_loudness(nullptr, (const float*)df.p, (const int64_t*)d0.p, (const PauseRec*)dr.p, n_rec, frame0[n_rec], (float*)dl.p));
  RVB_TRY(pause_cuts(nullptr, (const float*)dl.p, (const PauseRec*)dr.p, n_rec, chunk_size, search, h, (int32_t*)dt.p, (int32_t*)dc.p));
  if (hipDeviceSynchronize() != hipSuccess) { set_error(std::string(who) + ": a kernel failed"); return E_HIP; }
  std::vector<int32_t> table((size_t)std::max<int64_t>(tab, 1)), cnt(n_rec);
  if (tab) RVB_HIP_CHECK(hipMemcpy(table.data(), dt.p, (size_t)tab * 4, hipMemcpyDeviceToHost));
  RVB_HIP_CHECK(hipMemcpy(cnt.data(), dc.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
  int64_t total = 0;
  for (int r = 0; r < n_rec; ++r) {
    if (cnt[r] < 0 || cnt[r] > rec[r].tab_cap) { set_error(std::string(who) + ": the cut search left its table"); return E_HIP; }
    total += cnt[r];
  }
  if (total > capacity) { set_error(std::string(who) + ": capacity " + std::to_string(capacity) + " is too small: " + std::to_string(total) + " pieces"); return E_ARG; }
  int64_t k = 0;
  for (int r = 0; r < n_rec; ++r) {
    counts[r] = cnt[r];
    for (int j = 0; j < cnt[r]; ++j) starts[k++] = table[rec[r].tab0 + j];
  }
  return OK;
}

extern "C" int rvb_test_gather_chunks(const float* feats, int64_t n_rows, const int64_t* src, const int32_t* lens, int64_t n_pieces,
                                      int chunk_size, float* out) {
  const char* who = "rvb_test_gather_chunks";
  if (!feats || !src || !lens || !out || n_rows < 1 || n_pieces < 1 || n_pieces > (1 << 20) || chunk_size < 7 || chunk_size > (1 << 20)) {
    set_error(std::string(who) + ": bad argument"); return E_ARG;
  }
  std::vector<PausePiece> pieces((size_t)n_pieces);
  for (int64_t k = 0; k < n_pieces; ++k) {
    if (src[k] < 0 || lens[k] < 0 || lens[k] > chunk_size || src[k] + lens[k] > n_rows) {
      set_error(std::string(who) + ": piece " + std::to_string(k) + " lies outside the " + std::to_string(n_rows) + " rows or exceeds chunk_size"); return E_ARG;
    }
    pieces[k] = PausePiece{src[k], lens[k], 0};
  }
  RVB_TRY(need_device(who));
  const size_t out_bytes = (size_t)(n_pieces * chunk_size + 1) * 80 * 4;       // one sentinel row behind the last slot
  HipMem df, dp, dout;
  RVB_TRY(df.alloc(who, (size_t)n_rows * 80 * 4));
  RVB_TRY(dp.alloc(who, pieces.size() * sizeof(PausePiece)));
  RVB_TRY(dout.alloc(who, out_bytes));
  RVB_HIP_CHECK(hipMemcpy(df.p, feats, (size_t)n_rows * 80 * 4, hipMemcpyHostToDevice));
  RVB_HIP_CHECK(hipMemcpy(dp.p, pieces.data(), pieces.size() * sizeof(PausePiece), hipMemcpyHostToDevice));
  RVB_HIP_CHECK(hipMemset(dout.p, 0xff, out_bytes));
  RVB_TRY(pause_gather(nullptr, (const float*)df.p, (const PausePiece*)dp.p, n_pieces, chunk_size, (float*)dout.p));
  if (hipDeviceSynchronize() != hipSuccess) { set_error(std::string(who) + ": the kernel failed"); return E_HIP; }
  RVB_HIP_CHECK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return OK;
}
